"""numpy restatement of the arithmetic include/mnas.h specifies for global-norm clipping and the weight EMA (not a test: imported by
tests/test_gradclip_cpu.py and the -m gpu tests).

    norm = fp32( sqrt( float64 sum of ((float64) fp32(g[i] * grad_scale))^2 ) )          one rounding of the final value
    coef = 1, or with a finite max_norm > 0:  min(1, fp32(max_norm) / (norm + fp32(1e-6)))  in fp32, NaN kept (torch.clamp)
    ema  = d * ema + (1 - d) * p          (the kernels: fmaf(d, ema, fp32((1 - d) * p)); the tests bound it per element)
"""
import numpy as np

F32 = np.float32


def scaled(g, grad_scale=1.0):
    """the gradient the optimizer consumes: the fp32 product g[i] * grad_scale"""
    return (np.asarray(g, dtype=F32) * F32(grad_scale)).astype(F32)


def sqsum(g, grad_scale=1.0):
    """float64 sum of the squares of the fp32 products (each square is exact in float64)"""
    d = scaled(g, grad_scale).astype(np.float64)
    return float(np.sum(d * d, dtype=np.float64))


def norm(g, grad_scale=1.0):
    """the norm of one or several runs (a list / tuple of arrays is the norm of their concatenation)"""
    runs = g if isinstance(g, (list, tuple)) else [g]
    return F32(np.sqrt(np.float64(sum(sqsum(r, grad_scale) for r in runs))))


def coef(nrm, max_norm):
    """clip coefficient in fp32; max_norm None, <= 0 or +inf: 1"""
    if max_norm is None or not (max_norm > 0) or np.isinf(max_norm):
        return F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        q = F32(max_norm) / (F32(nrm) + F32(1e-6))
    return q if (q < F32(1.0) or np.isnan(q)) else F32(1.0)


def clipped(g, max_norm, grad_scale=1.0):
    """(norm, coef, fp32 (g * grad_scale) * coef)"""
    n = norm(g, grad_scale)
    c = coef(n, max_norm)
    return n, c, (scaled(g, grad_scale) * c).astype(F32)


def ema_bound(d, ema_prev, p_new):
    """(value, bound): d * ema + (1 - d) * p in float64 and the two-rounding fp32 bound 2^-23 (|d ema| + |(1 - d) p|) around it.
    d is the fp32 decay the kernel receives; 1 - d is formed in fp32 as the kernel forms it."""
    d32 = F32(d)
    dd, od = np.float64(d32), np.float64(F32(1.0) - d32)
    e, p = np.asarray(ema_prev, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return dd * e + od * p, 2.0 ** -23 * (np.abs(dd * e) + np.abs(od * p))
