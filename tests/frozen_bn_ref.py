"""Reference for training on FROZEN BatchNorm statistics (model.train(); features.eval()) -- TEST INFRASTRUCTURE.

The forward is the bf16 mirror's eval forward (oracle.bf16_mirror.conv_fwd(train=False): normalise with the running buffers, same
rounding points as the HIP path); the backward restates oracle.bf16_mirror.run's loop for statistics that are CONSTANTS of the step:

    dz = g * [s*y + t > 0]          S1 = sum dz          S2 = sum dz * (y*invstd - running_mean*invstd)
    dy = s * dz                     (the train-mode c2*y + c3 terms are the derivative of the batch statistics: gone)
    d bn.weight += S2     d bn.bias += S1     d conv.bias += s * S1     (not zero: nothing cancels the bias here)

The mirror's own conv_bwd hard-codes the batch-statistics formula, so the layer backward is written out here; the squeeze-excite
stage (se_fwd / se_bwd) has no BatchNorm and is reused as it is.  tests/test_frozen_bn_cpu.py pins this file to fp32 autograd through
oracle.features_forward(train=False)."""
import torch

from oracle import bf16_mirror as M
from oracle.mnasnet_oracle import round_bf16


def conv_bwd(saved, g, grads, resid=None, need_gin=True, se=None):
    """oracle.bf16_mirror.conv_bwd under frozen statistics (same arguments, same rounding points)."""
    spec, a, w, y, s, t = saved["spec"], saved["a"], saved["w"], saved["y"], saved["s"], saved["t"]
    mean, invstd = saved["mean"], saved["invstd"]          # eval forward: the running mean and 1/sqrt(running_var + eps)
    v = lambda c: c.view(1, -1, 1, 1)
    dz = g * ((y * v(s) + v(t)) > 0)
    xhat = y * v(invstd) + v(-mean * invstd)
    S1 = dz.double().sum((0, 2, 3))
    S2 = (dz * xhat).double().sum((0, 2, 3))
    dy = v(s) * dz
    if spec.kind != "dw":
        dy = round_bf16(dy)                 # staged as bf16 for the MFMA kernels; the depthwise kernels keep fp32
    p = spec.prefix

    def acc(name, val):
        grads[name] = grads.get(name, 0) + val

    acc(p + ".bn.weight", S2.float())
    acc(p + ".bn.bias", S1.float())
    acc(p + ".conv.bias", (s.double() * S1).float())
    if se is not None:                      # excitation applied on load: per-image slabs on the ungated activation (mirror's conv_bwd)
        sg = se["sg"]
        Pn = torch.einsum("nohw,nchw->noc", dy.double(), round_bf16(se["a"]).double())
        acc(p + ".conv.weight", (Pn * sg[:, None, :].double()).sum(0).float().view(tuple(w.shape)))
        W32 = saved["w32"].double().view(1, w.shape[0], w.shape[1])
        se["du"] = ((Pn * W32).sum(1) * (sg * (1 - sg)).double()).float()
    else:
        acc(p + ".conv.weight", torch.nn.grad.conv2d_weight(a, tuple(w.shape), dy, stride=spec.stride, padding=spec.pad,
                                                            groups=spec.groups))
    if not need_gin:
        return None
    gin = torch.nn.grad.conv2d_input(saved["in_shape"], w, dy, stride=spec.stride, padding=spec.pad, groups=spec.groups)
    if resid is not None:
        gin = gin + resid
    return gin if saved.get("image") else round_bf16(gin)


def run(program, st, x, cot=None, need_dx=False, se_on_load=None):
    """oracle.bf16_mirror.run for the frozen mode: same program / state / arguments; ``st`` is not modified.
    Returns dict(y=fp32 output, grads={name: tensor}, dx=fp32 or None)."""
    first = program[0][1] if program[0][0] == "conv" else program[0][1][0]
    is_image = first.kind == "dense" and first.cin == 3
    cur = None if is_image else M.MAct(round_bf16(x))
    tape = []
    for op, arg in program:
        if op == "conv":
            cur, sv = M.conv_fwd(arg, cur, st, False, image=x if (cur is None) else None)
            tape.append(("conv", sv))
        else:
            a_in = cur
            h = cur
            svs = []
            N_, C_, H_, W_ = a_in.data.shape
            sse = None
            for j, spec in enumerate(arg[:3]):
                if j == 2 and len(arg) == 4:
                    h, sse = M.se_fwd(arg[3], h, st)
                    sse["on_load"] = bool(se_on_load and se_on_load(N_, H_, W_, h.data.shape[1]))
                h, sv = M.conv_fwd(spec, h, st, False)
                svs.append(sv)
            svs.append(sse)
            cur = M.MAct(round_bf16(a_in.f32() + h.f32()))
            tape.append(("block", svs))
    out = dict(y=cur.f32(), grads={}, dx=None)
    if cot is None:
        return out
    g = round_bf16(cot)
    grads = out["grads"]
    for n in range(len(tape) - 1, -1, -1):
        kind, sv = tape[n]
        first_step = n == 0
        if kind == "conv":
            need = (not first_step) or need_dx
            g = conv_bwd(sv, g, grads, None, need)
        else:
            G = g
            g2 = conv_bwd(sv[2], G, grads, se=sv[3] if (sv[3] is not None and sv[3]["on_load"]) else None)
            if sv[3] is not None:
                g2 = M.se_bwd(sv[3], g2, grads)
            g1 = conv_bwd(sv[1], g2, grads)
            need = (not first_step) or need_dx
            g = conv_bwd(sv[0], g1, grads, G if need else None, need)
    out["dx"] = g
    return out
