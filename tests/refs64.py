"""fp64 references built from slicing, matmul and elementwise ops only (no convolution call: nothing goes to a vendor convolution
library on the device).  NHWC layouts as the kernels use them; `device` is where the fp64 math runs."""
import torch


def f64(t, device):
    return t.to(device=device, dtype=torch.float64)


def pad_hw(x, p):
    """zero-pad an NHWC tensor by p rows / columns on each side"""
    if p == 0:
        return x
    N, H, W, C_ = x.shape
    out = torch.zeros((N, H + 2 * p, W + 2 * p, C_), dtype=x.dtype, device=x.device)
    out[:, p:p + H, p:p + W] = x
    return out


def ref_dy(g, y, coef, device="cpu"):
    """dy = c1*g*[s*y+t > 0] + c2*y + c3 over the last (channel) dimension; coef: bnbuf rows 0..4 ([>=5][C])"""
    g, y, cf = f64(g, device), f64(y, device), f64(coef, device)
    s, t, c1, c2, c3 = cf[0], cf[1], cf[2], cf[3], cf[4]
    return c1 * g * ((s * y + t) > 0) + c2 * y + c3


def ref_dw_fwd(x, w, bias=None, stride=1, device="cpu"):
    """depthwise k x k, pad k//2, stride 1 or 2: x (N,H,W,C), w (C,k,k) -> (N,Ho,Wo,C)"""
    x, w = f64(x, device), f64(w, device)
    N, H, W, C_ = x.shape
    k = w.shape[-1]
    xp = pad_hw(x, k // 2)
    y = torch.zeros_like(x)
    for kh in range(k):
        for kw in range(k):
            y += xp[:, kh:kh + H, kw:kw + W] * w[:, kh, kw]
    y = y[:, ::stride, ::stride].contiguous()
    if bias is not None:
        y += f64(bias, device)
    return y


def ref_dw_dgrad(dy, w, H=None, W=None, stride=1, device="cpu"):
    """input gradient of ref_dw_fwd: dy (N,Ho,Wo,C) -> (N,H,W,C) (H, W default to dy's: stride 1)"""
    dy, w = f64(dy, device), f64(w, device)
    N, Ho, Wo, C_ = dy.shape
    H, W = Ho if H is None else H, Wo if W is None else W
    k = w.shape[-1]
    p = k // 2
    gp = torch.zeros((N, max(H + 2 * p, (Ho - 1) * stride + k), max(W + 2 * p, (Wo - 1) * stride + k), C_), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            gp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] += dy * w[:, kh, kw]
    return gp[:, p:p + H, p:p + W].contiguous()


def ref_dw_wgrad(x, dy, k, stride=1, device="cpu"):
    """weight gradient of ref_dw_fwd: x (N,H,W,C), dy (N,Ho,Wo,C) -> (C,k,k)"""
    x, dy = f64(x, device), f64(dy, device)
    N, H, W, C_ = x.shape
    _, Ho, Wo, _ = dy.shape
    xp = pad_hw(x, k // 2)
    dw = torch.zeros((C_, k, k), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            dw[:, kh, kw] = (xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] * dy).sum((0, 1, 2))
    return dw


def ref_dense_fwd(a, w, bias=None, stride=1, pad=None, device="cpu"):
    """dense k x k conv: a (N,H,W,Ci) (the operand as the kernel sees it), w (Co,Ci,k,k), bias [Co] -> (N,Ho,Wo,Co).
    One matmul per tap over a strided slice of the zero-padded input."""
    a, w = f64(a, device), f64(w, device)
    N, H, W, Ci = a.shape
    Co, _, k, _ = w.shape
    p = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    ap = pad_hw(a, p)
    y = torch.zeros((N, Ho, Wo, Co), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            y += torch.matmul(ap[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride], w[:, :, kh, kw].t())
    if bias is not None:
        y += f64(bias, device)
    return y


def ref_dense_dgrad(dy, w, H, W, stride=1, pad=None, device="cpu"):
    """input gradient of ref_dense_fwd: dy (N,Ho,Wo,Co), w (Co,Ci,k,k) -> (N,H,W,Ci) (any stride).  Forward pixel ho reads input
    row stride*ho + kh - pad, so tap (kh, kw) scatters dy[ho, wo] @ w[:, :, kh, kw] to padded row stride*ho + kh."""
    dy, w = f64(dy, device), f64(w, device)
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
    a, dy = f64(a, device), f64(dy, device)
    N, H, W, Ci = a.shape
    _, Ho, Wo, Co = dy.shape
    ap = pad_hw(a, k // 2 if pad is None else pad)
    dw = torch.zeros((Co, Ci, k, k), dtype=torch.float64, device=device)
    d2 = dy.reshape(-1, Co)
    for kh in range(k):
        for kw in range(k):
            sl = ap[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            dw[:, :, kh, kw] = d2.t() @ sl.reshape(-1, Ci)
    return dw


def ref_stem(t, w, bias=None, device="cpu"):
    """the stem conv (3x3, stride 2, pad 1) over the image the kernel stages: t (N,3,H,W) NCHW, w (Co,3,3,3) -> (N,Ho,Wo,Co)"""
    return ref_dense_fwd(t.permute(0, 2, 3, 1), w, bias, stride=2, pad=1, device=device)


def ref_stem_wgrad(t, dy, device="cpu"):
    """t (N,3,H,W), dy (N,Ho,Wo,Co) -> (Co,3,3,3)"""
    return ref_dense_wgrad(t.permute(0, 2, 3, 1), dy, 3, stride=2, pad=1, device=device)
