"""Plain torch-CPU statements of the grouped AdamW step and the weight EMA of csrc/optim_groups.hip, and the helpers the
tests of those kernels share.  No GPU is touched here and the package is not imported; tests/test_optim_groups_cpu.py
checks this file.

The grouped step IS tests/optim_ref.py's ``adam_step`` (decoupled decay, device bias correction) applied to each group's
elements with the group's rate and decay; the rate of group g is formed as the kernel forms it, ``f32(f32(lr) *
f32(lr_scale_g))``.  The tolerance is optim_ref's (``check_adam`` with its documented K), applied to each group's elements;
nothing is added to it here.  The EMA statement is timm's ModelEmaV2, ``ema = d ema + (1 - d) p``, held to
``rowwise_ref.assert_close`` with the fp32 statement as the chain and max(|ema|, |p|) as the operand magnitude."""
from __future__ import annotations

import torch

from tests import optim_ref as O
from tests.rowwise_ref import assert_close, fp32_chain, ref64

SCALES = (1.0, 0.75, 2.0 ** -5)
DECAYS = (0.09, 0.0, 0.05)


def group_lr(lr, scale) -> float:
    """the rate of a group as the kernel forms it: both factors rounded to fp32, their product rounded to fp32"""
    return O.f32(O.f32(lr) * O.f32(scale))


def interleaved_groups(n, ngroups=3):
    """uint8 [ceil(n / 64)]: the groups laid over the 64-blocks as 0, 1, .., ngroups - 1, .., 1, 0, 1, ..  (0, 1, 2, 1, 0, ...)"""
    nb = (n + 63) // 64
    period = max(2 * (ngroups - 1), 1)
    idx = torch.arange(nb) % period
    return torch.where(idx < ngroups, idx, period - idx).to(torch.uint8)


def group_elements(group64, gi, n):
    """indices of the elements of group ``gi``, block after block (so a 64-block skip mask restricted to the group's blocks
    still lines up: the only partial block is the buffer's last one, which comes last)"""
    blocks = (group64 == gi).nonzero().flatten()
    idx = (blocks[:, None] * 64 + torch.arange(64)[None, :]).flatten()
    return blocks, idx[idx < n]


def groups_step(p, g, m, v, group64, scales, decays, *, lr, b1, b2, eps, steps_taken, skip=None):
    """one grouped AdamW step -> (p, m, v) in the dtype handed: ``optim_ref.adam_step`` per group"""
    n = p.numel()
    out = [p.clone(), m.clone(), v.clone()]
    for gi, (s, wd) in enumerate(zip(scales, decays)):
        blocks, idx = group_elements(group64, gi, n)
        if idx.numel() == 0:
            continue
        new = O.adam_step(p[idx], g[idx], m[idx], v[idx], lr=group_lr(lr, s), b1=b1, b2=b2, eps=eps, wd=wd,
                          steps_taken=steps_taken, coupled=False, bias="device")
        sk = None if skip is None else skip[blocks]
        for o, old, x in zip(out, (p, m, v), new):
            o[idx] = O.apply_skip(old[idx], x, sk)
    return tuple(out)


def check_groups(got, inputs, group64, scales, decays, hyper, *, K=None, skip=None, what=""):
    """``optim_ref.check_adam`` on each group's elements with that group's rate and decay -> the worst error / budget"""
    n = inputs[0].numel()
    worst = None
    for gi, (s, wd) in enumerate(zip(scales, decays)):
        blocks, idx = group_elements(group64, gi, n)
        if idx.numel() == 0:
            continue
        h = dict(hyper, lr=group_lr(hyper["lr"], s), wd=wd, coupled=False, bias="device")
        r = O.check_adam(tuple(t[idx] for t in got), tuple(t[idx] for t in inputs), h, K=K,
                         skip=None if skip is None else skip[blocks], what=f"{what} group {gi}")
        worst = r if worst is None else {k: max(worst[k], r[k]) for k in r}
    return worst


def ema_step(ema, p, *, d):
    """timm ModelEmaV2: ema = d ema + (1 - d) p, d rounded to fp32 first, in the dtype handed"""
    d = torch.tensor(O.f32(d), dtype=ema.dtype)
    return d * ema + (1 - d) * p


def check_ema(got, ema, p, d, what=""):
    """the EMA a kernel left against the float64 statement, under rowwise_ref's rule"""
    mag = torch.maximum(ema.double().abs(), p.double().abs())
    assert_close(got, ref64(ema_step, ema, p, d=d), fp32_chain(ema_step, ema, p, d=d), mag, what)
