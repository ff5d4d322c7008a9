"""fp64 numpy reference of the grouped optimizer steps (include/mnas.h: mnas_*_step_seg): decoupled weight decay (AdamW: Loshchilov
& Hutter, "Decoupled Weight Decay Regularization"), LAMB (You et al., "Large Batch Optimization for Deep Learning: Training BERT in
76 minutes", algorithm 2, with the bias correction and without a clamp on the weight norm) and LARS (You, Gitman & Ginsburg, "Large
Batch Training of Convolutional Networks", with the trust coefficient and an epsilon in the denominator).  It restates the formulas
from the papers and shares no code with the package.  Every function takes and returns float64 arrays; `segments` is a list of
(begin, end, group index or None for a frozen tensor) over the flat arrays, `groups` a list of dicts lr / wd / trust."""
import numpy as np


def f64(x):
    return np.asarray(x, dtype=np.float64)


def norm(x):
    """sqrt(sum x^2) in float64"""
    x = f64(x).ravel()
    return float(np.sqrt(np.sum(x * x)))


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step):
    """one AdamW step: the decay multiplies the weights ahead of an Adam update that sees the undecayed gradient"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    mhat, vhat = m / (1.0 - b1 ** step), v / (1.0 - b2 ** step)
    return p - lr * mhat / (np.sqrt(vhat) + eps), m, v


def lamb_direction(p, g, m, v, b1, b2, eps, wd, step):
    """(u, m', v'): u = mhat / (sqrt(vhat) + eps) + wd p"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    mhat, vhat = m / (1.0 - b1 ** step), v / (1.0 - b2 ** step)
    return mhat / (np.sqrt(vhat) + eps) + wd * p, m, v


def lamb_ratio(w, un):
    """phi(||w||) / ||u|| with phi the identity; 1 where either norm is zero"""
    return w / un if (w > 0 and un > 0) else 1.0


def lars_ratio(w, gn, wd, coef, eps):
    """local learning-rate factor  coef ||w|| / (||g|| + wd ||w|| + eps); 1 where either norm is zero"""
    return coef * w / (gn + wd * w + eps) if (w > 0 and gn > 0) else 1.0


def lamb_step(p, g, m, v, segments, groups, b1, b2, eps, step):
    """-> (p', m', v', {segment index: (w, un, r)}); frozen segments untouched and absent from the dict"""
    p, g, m, v = (f64(t).copy() for t in (p, g, m, v))
    out = {}
    for k, (a, b, gi) in enumerate(segments):
        if gi is None:
            continue
        gr = groups[gi]
        u, m[a:b], v[a:b] = lamb_direction(p[a:b], g[a:b], m[a:b], v[a:b], b1, b2, eps, gr["wd"], step)
        w, un = norm(p[a:b]), norm(u)
        r = lamb_ratio(w, un) if gr["trust"] else 1.0
        out[k] = (w, un, r)
        p[a:b] = p[a:b] - gr["lr"] * r * u
    return p, m, v, out


def lars_step(p, g, buf, segments, groups, momentum, dampening, nesterov, first, coef, eps):
    """-> (p', buf', {segment index: (w, gn, r)}): the decayed gradient is scaled by the local factor, then momentum SGD"""
    p, g, buf = (f64(t).copy() for t in (p, g, buf))
    out = {}
    for k, (a, b, gi) in enumerate(segments):
        if gi is None:
            continue
        gr = groups[gi]
        w, gn = norm(p[a:b]), norm(g[a:b])
        r = lars_ratio(w, gn, gr["wd"], coef, eps) if gr["trust"] else 1.0
        out[k] = (w, gn, r)
        d = (g[a:b] + gr["wd"] * p[a:b]) * r
        if momentum != 0.0:
            buf[a:b] = d if first else momentum * buf[a:b] + (1.0 - dampening) * d
            d = d + momentum * buf[a:b] if nesterov else buf[a:b]
        p[a:b] = p[a:b] - gr["lr"] * d
    return p, buf, out
