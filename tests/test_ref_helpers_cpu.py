"""CPU self-test of the fp64 references in tests/refs64.py (used by tests/test_gpu_bwd_forms.py on the device): each one
against torch.nn.functional / torch.nn.grad in fp64 at small shapes, odd planes and both depthwise kernel sizes, to 1e-12.
Also the guarded-buffer helper's two checks (a write outside the view, an element never written)."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import bits_equal, guarded
from intervals import Interval
from refs64 import ref_dense_dgrad, ref_dw_dgrad, ref_dw_fwd, ref_dw_wgrad, ref_dy


def _r(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _close(a, b):
    err = float((a - b).abs().max() / (b.abs().max() + 1e-300))
    assert err < 1e-12, err


@pytest.mark.parametrize("N,H,W,C_,k", [(2, 7, 9, 8, 3), (1, 5, 4, 16, 5), (3, 1, 6, 8, 3), (2, 6, 6, 24, 5)])
def test_depthwise_references(N, H, W, C_, k):
    x, dy, w = _r((N, H, W, C_), 1), _r((N, H, W, C_), 2), _r((C_, k, k), 3)
    w4 = w.view(C_, 1, k, k)
    _close(_nchw(ref_dw_fwd(x, w)), F.conv2d(_nchw(x), w4, padding=k // 2, groups=C_))
    _close(_nchw(ref_dw_dgrad(dy, w)),
           torch.nn.grad.conv2d_input((N, C_, H, W), w4, _nchw(dy), padding=k // 2, groups=C_))
    _close(ref_dw_wgrad(x, dy, k),
           torch.nn.grad.conv2d_weight(_nchw(x), (C_, 1, k, k), _nchw(dy), padding=k // 2, groups=C_).view(C_, k, k))


@pytest.mark.parametrize("N,H,W,C_,k,stride", [(2, 7, 9, 8, 3, 2), (1, 6, 4, 16, 5, 2), (2, 5, 5, 8, 5, 1), (2, 8, 8, 8, 3, 2)])
def test_strided_depthwise_gradient_references(N, H, W, C_, k, stride):
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    x, dy, w = _r((N, H, W, C_), 1), _r((N, Ho, Wo, C_), 2), _r((C_, k, k), 3)
    w4 = w.view(C_, 1, k, k)
    _close(_nchw(ref_dw_dgrad(dy, w, H, W, stride)),
           torch.nn.grad.conv2d_input((N, C_, H, W), w4, _nchw(dy), stride=stride, padding=p, groups=C_))
    _close(ref_dw_wgrad(x, dy, k, stride),
           torch.nn.grad.conv2d_weight(_nchw(x), (C_, 1, k, k), _nchw(dy), stride=stride, padding=p, groups=C_).view(C_, k, k))


def test_interval_identities():
    lo = _r((40, 8), 9)
    iv = Interval(lo, lo + _r((40, 8), 10).abs())
    assert torch.allclose(iv.amax, iv.mid.abs() + iv.half, rtol=0, atol=1e-15)       # what wgrad_terms' slack relies on
    assert bool((iv.mid - iv.half - iv.lo).abs().max() < 1e-15)


@pytest.mark.parametrize("N,H,W,Ci,Co", [(2, 8, 10, 16, 24), (1, 7, 9, 8, 16), (3, 14, 14, 24, 8), (2, 2, 2, 8, 8), (1, 1, 3, 8, 8)])
def test_dense_s2_dgrad_reference(N, H, W, Ci, Co):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy, w = _r((N, Ho, Wo, Co), 4), _r((Co, Ci, 3, 3), 5)
    ref = torch.nn.grad.conv2d_input((N, Ci, H, W), w, _nchw(dy), stride=2, padding=1)
    _close(_nchw(ref_dense_dgrad(dy, w, H, W, stride=2, pad=1)), ref)


def test_dy_reference():
    g, y = _r((5, 7, 16), 6), _r((5, 7, 16), 7)
    coef = _r((8, 16), 8)
    s, t, c1, c2, c3 = coef[:5]
    want = c1 * torch.where(s * y + t > 0, g, torch.zeros_like(g)) + c2 * y + c3
    _close(ref_dy(g, y, coef), want)
    assert bool(((s * y + t) <= 0).any()) and bool(((s * y + t) > 0).any())      # both sides of the mask exercised


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guarded_detects_stray_and_missing_writes(dtype):
    v, check = guarded((3, 5), dtype, device="cpu")
    with pytest.raises(AssertionError, match="never written"):
        check()
    v.fill_(1.0)
    check()
    v.view(-1)[7] = float("nan")                # a NaN the kernel computed is not the fill pattern
    check()
    base = v.view(-1)
    base.as_strided((1,), (1,), base.storage_offset() + 15).fill_(0.0)      # one element past the end
    with pytest.raises(AssertionError, match="past the end"):
        check()


def test_bits_equal():
    a = torch.tensor([1.0, 0.0, -2.5], dtype=torch.bfloat16)
    b = torch.tensor([1.0, -0.0, -2.5], dtype=torch.bfloat16)
    bits_equal(a, b, signed_zero=False)
    with pytest.raises(AssertionError, match="differ"):
        bits_equal(a, b)
    with pytest.raises(AssertionError, match=r"\(2,\)"):
        bits_equal(a, torch.tensor([1.0, 0.0, -2.0], dtype=torch.bfloat16))
