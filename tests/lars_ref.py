"""A restatement of the LARS update rule (pl_bolts' public ``LARS.step``) in torch on the CPU, independent of the HIP kernels.

``lars_step`` takes the working dtype (float64: the reference chain; float32: the same rule with every operation rounded
in fp32) and the order in which the squares of a norm are added:

    order="tensor"   one sum over the whole tensor (torch's pairwise sum)
    order="chunks"   sums over consecutive chunks of ``chunk`` elements, then the sum of those (how a chunked reduction
                     associates; the chunk length comes from ``ops.lars_plan``)

Per parameter with a gradient:

    d = g
    if weight_decay != 0 and |p| != 0 and |g| != 0:
        d = trust_coefficient |p| / (|g| + weight_decay |p| + eps) * (g + weight_decay p)
    if momentum != 0:
        buf = d on the parameter's first step, momentum buf + (1 - dampening) d afterwards
        d = d + momentum buf if nesterov else buf
    p = p - lr d
"""
import torch


def _norm(t, order, chunk):
    sq = t.reshape(-1) * t.reshape(-1)
    if order == "tensor":
        return sq.sum().sqrt()
    if order != "chunks":
        raise ValueError(order)
    return torch.stack([c.sum() for c in sq.split(chunk)]).sum().sqrt()


def lars_step(params, grads, bufs, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
              trust_coefficient=0.001, eps=1e-8, dtype=torch.float64, order="tensor", chunk=8192):
    """One step.  params / grads / bufs: lists of tensors (any float dtype; a grad of None skips that parameter; a buf of
    None means the parameter has not stepped yet).  weight_decay: a float or one value per parameter.
    -> (new params, new bufs) in ``dtype``; the inputs are not modified."""
    wds = [weight_decay] * len(params) if isinstance(weight_decay, (int, float)) else list(weight_decay)
    c = lambda v: torch.tensor(v, dtype=dtype)
    out_p, out_b = [], []
    for p, g, buf, wd in zip(params, grads, bufs, wds):
        p = p.to(dtype)
        if g is None:
            out_p.append(p.clone())
            out_b.append(None if buf is None else buf.to(dtype).clone())
            continue
        g = g.to(dtype)
        d = g
        pn, gn = _norm(p, order, chunk), _norm(g, order, chunk)
        if wd != 0 and pn != 0 and gn != 0:
            q = c(trust_coefficient) * pn / (gn + c(wd) * pn + c(eps))
            d = q * (g + c(wd) * p)
        if momentum != 0:
            buf = d.clone() if buf is None else c(momentum) * buf.to(dtype) + c(1.0 - dampening) * d
            d = d + c(momentum) * buf if nesterov else buf
        out_p.append(p - c(lr) * d)
        out_b.append(buf)
    return out_p, out_b
