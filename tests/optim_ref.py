"""Plain torch-CPU statements of ONE step of every streaming optimizer kernel of csrc/optim.hip from a handed state, the
input recipe and the tolerance rule of tests/test_gpu_optim.py.  No GPU is touched here and the package is not imported;
tests/test_optim_cpu.py checks this file.

Every step is one function of tensors that works in the dtype it is handed, so ``rowwise_ref.ref64`` evaluates it in float64
(the reference) and ``rowwise_ref.fp32_chain`` in fp32 (the arithmetic contract of the kernels).  Hyperparameters are rounded
to fp32 first in both precisions: the kernels receive floats, and the reference must see the operands the kernel sees.

The tolerance.  Everything is compared after one step from a handed state, never after a trajectory: a second consecutive
launch starts from the GPU's own state read back, which the test hands to the reference.  The base rule is
``rowwise_ref.assert_close``: per element, four times the fp32 chain's own worst error on these inputs plus one fp32 ulp, in
units of the spacing at the largest magnitude behind that element (``*_mags`` below).  Device sqrtf and / are correctly
rounded at the project's build flags and the kernel's fmafs only drop roundings the chain has, so a kernel fed by the host's
bias correction (``bias="host"``: dvt_adamw_step) needs nothing more.

A kernel that reads the step counter (``bias="device"``) forms 1 - b1^t and sqrt(1 - b2^t) with the device's powf, which the
chain (torch's CPU pow) does not bound: 1 - b^t cancels, so one ulp of powf becomes hundreds of ulps of the update at
b2 = 0.999, t <= 10.  The parametrisation of the tests is therefore three regimes (``REGIMES``):
  * powers negligible (b1 0.9, b2 0.999, 30 000 and 100 000 steps: both powers below 2^-28): the base rule alone; this
    carries the elementwise precision at the workload's betas;
  * powers small (b1 2^-4, b2 2^-5, t = 1, 2, 3: the powers are exact): the base rule plus the scalar term below, there
    under 1.6e-7 relative -- a wrong t and a missing or misplaced correction are caught tightly;
  * workload betas, first steps (t = 1, 2, 10, 1000): the base rule plus the scalar term
        E_i += |update_ref,i| * K * ( ulp32(b1^t) / (1 - b1^t) + ulp32(b2^t) / (2 (1 - b2^t)) ),   on p only,
    with K = ``POWF_ULPS`` = 16.  K is a CAP, NOT A MEASUREMENT: 16 ulp is the OpenCL full-profile bound for pow, the
    loosest published bound for the math library the kernels compile against.  The error of the device's powf has not
    been measured in this project.  The term costs 5e-4 relative at t = 1; the faults this regime exists for (a wrong t,
    a missing correction) change the update by 5 % and more.
16-bit mirrors are not a tolerance question: a mirror equals the fp32 parameter the same launch wrote, cast, bit for bit."""
from __future__ import annotations

import math

import torch

from tests.rowwise_ref import assert_close, budget, fp32_chain, ref64, ulp32

POWF_ULPS = 16.0

# name -> (b1, b2, steps_taken, K of the scalar term or None)
REGIMES = {
    "negligible-29999": (0.9, 0.999, 29999, None),
    "negligible-99999": (0.9, 0.999, 99999, None),
    "small-0": (2.0 ** -4, 2.0 ** -5, 0, POWF_ULPS),
    "small-1": (2.0 ** -4, 2.0 ** -5, 1, POWF_ULPS),
    "small-2": (2.0 ** -4, 2.0 ** -5, 2, POWF_ULPS),
    "workload-0": (0.9, 0.999, 0, POWF_ULPS),
    "workload-1": (0.9, 0.999, 1, POWF_ULPS),
    "workload-9": (0.9, 0.999, 9, POWF_ULPS),
    "workload-999": (0.9, 0.999, 999, POWF_ULPS),
}


def f32(x) -> float:
    """a Python number (or one-element tensor) rounded to fp32"""
    return float(torch.as_tensor(x, dtype=torch.float64).reshape(()).to(torch.float32))


def _scalars(like, *xs):
    return tuple(torch.tensor(f32(x), dtype=like.dtype) for x in xs)


# ---------------------------------------------------------------- Adam / AdamW
def bias_pair(b1, b2, steps_taken, dtype, bias):
    """(1 - b1^t, sqrt(1 - b2^t)) at t = steps_taken + 1 as scalars of ``dtype``.  "host": formed in float64 and rounded
    to fp32 whatever ``dtype`` is (dvt_adamw_step); "device": formed in ``dtype`` (every kernel that reads the counter)."""
    t = steps_taken + 1
    b1, b2 = f32(b1), f32(b2)
    if bias == "host":
        return torch.tensor(f32(1.0 - b1 ** t), dtype=dtype), torch.tensor(f32(math.sqrt(1.0 - b2 ** t)), dtype=dtype)
    assert bias == "device", bias
    tt = torch.tensor(float(t), dtype=dtype)
    return 1 - torch.pow(torch.tensor(b1, dtype=dtype), tt), torch.sqrt(1 - torch.pow(torch.tensor(b2, dtype=dtype), tt))


def adam_step(p, g, m, v, *, lr, b1, b2, eps, wd, steps_taken, coupled, bias):
    """one step of AdamW (``coupled`` False: p *= 1 - lr wd first) or torch.optim.Adam (True: g += wd p first)
    -> (p, m, v).  Denominator sqrt(v) / sqrt(1 - b2^t) + eps, step size lr / (1 - b1^t)."""
    bc1, bc2s = bias_pair(b1, b2, steps_taken, p.dtype, bias)
    lr, b1, b2, eps, wd = _scalars(p, lr, b1, b2, eps, wd)
    step_size = lr / bc1
    if coupled:
        g = g + wd * p
    else:
        p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    den = v.sqrt() / bc2s + eps
    return p - step_size * (m / den), m, v


def adam_mags(p, g, m, v, ref, *, lr, b1, b2, eps, wd, steps_taken, coupled, **_):
    """operand magnitudes behind each element of (p, m, v) and the float64 update |step_size m / den|.  The third term of
    the p magnitude matters where b1 m + (1 - b1) g cancels: the update is small there, its error is not."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    ref_p, ref_m, ref_v = (t.double() for t in ref)
    bc1, bc2s = bias_pair(b1, b2, steps_taken, torch.float64, "device")
    g_eff = g.abs() + (f32(wd) * p.abs() if coupled else 0.0)
    mag_m = torch.maximum(m.abs(), g_eff)
    mag_v = torch.maximum(v, g_eff * g_eff)
    step_size = f32(lr) / bc1
    den = ref_v.sqrt() / bc2s + f32(eps)
    spread = step_size * mag_m / den
    update = step_size * ref_m.abs() / den
    return torch.maximum(torch.maximum(p.abs(), ref_p.abs()), spread), mag_m, mag_v, update


def powf_term(update, b1, b2, steps_taken, K):
    """the scalar term of the docstring: what K ulps of error in each of the two powers may move p by"""
    t = steps_taken + 1
    x1, x2 = f32(b1) ** t, f32(b2) ** t
    rel = float(ulp32(torch.tensor(x1))) / (1 - x1) + float(ulp32(torch.tensor(x2))) / (2 * (1 - x2))
    return update * (K * rel)


def within(got, ref, chain32, mag, extra=None, what=""):
    """``rowwise_ref.budget`` (+ ``extra`` per element) on an fp32 tensor; -> the worst error as a fraction of its budget.
    Without ``extra`` this is ``rowwise_ref.assert_close`` itself, which is called as well."""
    if extra is None:
        assert_close(got, ref, chain32, mag, what)
    assert got.dtype == torch.float32 and got.shape == ref.shape, what
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    E = budget(ref, chain32, mag)
    if extra is not None:
        E = E + extra
    err = (got.double() - ref.double()).abs()
    ratio = err / E
    if got.numel() == 0:
        return 0.0
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the budget, worst "
                             f"{worst:.3g} x at {i}: got {float(got[i])!r}, reference {float(ref[i])!r}, E {float(E[i]):.3e}")
    return worst


def apply_skip(old, new, skip):
    """elements of 64-blocks whose mask byte is set keep ``old``"""
    if skip is None:
        return new
    mask = skip.bool().repeat_interleave(64)[:old.numel()]
    return torch.where(mask, old, new)


def check_adam(got, inputs, hyper, *, K=None, skip=None, what=""):
    """``got`` = (p, m, v) a kernel left, ``inputs`` = (p, g, m, v) it was handed (all fp32 on the CPU), ``hyper`` the
    keywords of ``adam_step``: every tensor within the rule.  -> {"p" / "m" / "v": worst error / budget}"""
    old = (inputs[0], inputs[2], inputs[3])
    ref = ref64(adam_step, *inputs, **hyper)
    chain = fp32_chain(adam_step, *inputs, **hyper)
    mag_p, mag_m, mag_v, update = adam_mags(*inputs, ref, **hyper)
    extra = None if K is None else apply_skip(torch.zeros_like(update), powf_term(update, hyper["b1"], hyper["b2"],
                                                                                 hyper["steps_taken"], K), skip)
    ref = tuple(apply_skip(o.double(), r, skip) for o, r in zip(old, ref))
    chain = tuple(apply_skip(o, c, skip) for o, c in zip(old, chain))
    out = {}
    for name, gt, r, c, mag, ex in zip("pmv", got, ref, chain, (mag_p, mag_m, mag_v), (extra, None, None)):
        out[name] = within(gt, r, c, mag, ex, f"{what} {name}")
    return out


# ---------------------------------------------------------------- SGD, Adagrad
def sgd_step(p, g, buf, *, lr, mu, wd):
    """torch.optim.SGD (dampening 0, no nesterov) -> (p, buf); mu == 0 leaves buf (which may be None) as it is"""
    lr_, mu_, wd_ = _scalars(p, lr, mu, wd)
    d = g + wd_ * p
    if f32(mu) == 0.0:
        return p - lr_ * d, buf
    buf = mu_ * buf + d
    return p - lr_ * buf, buf


def adagrad_clr(lr, lr_decay, step) -> float:
    return f32(f32(lr) / (1.0 + (step - 1) * f32(lr_decay)))


def adagrad_step(p, g, s, *, lr, lr_decay, eps, wd, step):
    """torch.optim.Adagrad -> (p, sum): d = g + wd p; sum += d^2; p -= clr d / (sqrt(sum) + eps)"""
    clr, eps_, wd_ = _scalars(p, adagrad_clr(lr, lr_decay, step), eps, wd)
    d = g + wd_ * p
    s = s + d * d
    return p - clr * (d / (s.sqrt() + eps_)), s


def check_sgd(got, inputs, hyper, *, skip=None, what=""):
    p, g, buf = inputs
    mom = f32(hyper["mu"]) != 0.0
    b0 = buf if mom else None
    rp, rb = ref64(sgd_step, p, g, b0, **hyper)
    cp, cb = sgd_step(p, g, b0, **hyper)
    d_mag = torch.maximum(g.double().abs(), f32(hyper["wd"]) * p.double().abs())
    mag_b = torch.maximum(buf.double().abs(), d_mag) if mom else d_mag
    out = {"p": within(got[0], apply_skip(p.double(), rp, skip), apply_skip(p, cp, skip),
                       torch.maximum(p.double().abs(), f32(hyper["lr"]) * mag_b), None, f"{what} p")}
    if mom:
        out["buf"] = within(got[1], apply_skip(buf.double(), rb, skip), apply_skip(buf, cb, skip), mag_b, None, f"{what} buf")
    return out


def check_adagrad(got, inputs, hyper, *, skip=None, what=""):
    p, g, s = inputs
    rp, rs = ref64(adagrad_step, p, g, s, **hyper)
    cp, cs = adagrad_step(p, g, s, **hyper)
    d_mag = torch.maximum(g.double().abs(), f32(hyper["wd"]) * p.double().abs())
    spread = adagrad_clr(hyper["lr"], hyper["lr_decay"], hyper["step"]) * d_mag / (rs.sqrt() + f32(hyper["eps"]))
    spread = torch.where(torch.isfinite(spread), spread, torch.zeros_like(spread))
    return {"p": within(got[0], apply_skip(p.double(), rp, skip), apply_skip(p, cp, skip),
                        torch.maximum(p.double().abs(), spread), None, f"{what} p"),
            "sum": within(got[1], apply_skip(s.double(), rs, skip), apply_skip(s, cs, skip),
                          torch.maximum(s.double(), d_mag * d_mag), None, f"{what} sum")}


# ---------------------------------------------------------------- the loss-scaled step as a state machine
def scaler_state(scale, steps=0, good_steps=0):
    """the device state of dvt_adamw_step_scaled before its first launch (loss_grad is written by the launch)"""
    return dict(steps=int(steps), scale=f32(scale), found_inf=0, good_steps=int(good_steps), loss_grad=None)


def scaled_step(p, g, m, v, state, *, lr, b1, b2, eps, wd, growth_interval, growth, backoff, base, skip=None):
    """the whole of dvt_adamw_step_scaled -> (p, m, v, state).  A non-finite gradient ANYWHERE -- inside a skipped block as
    well: the finiteness check reads the whole buffer -- means nothing moves, scale *= backoff, good_steps = 0.  Otherwise
    AdamW (device bias) runs on g / scale, the counter advances by one and the scale grows by ``growth`` every
    ``growth_interval`` clean steps (torch.amp.GradScaler's rule).  found_inf is left 0, loss_grad = scale * base.  The
    scaler's own arithmetic is fp32 whatever the dtype of the tensors."""
    st = dict(state)
    scale = torch.tensor(st["scale"], dtype=torch.float32)
    if st["found_inf"] or not bool(torch.isfinite(g).all()):
        scale = scale * torch.tensor(backoff, dtype=torch.float32)
        st["good_steps"] = 0
    else:
        new = adam_step(p, g / scale.to(p.dtype), m, v, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, steps_taken=st["steps"],
                        coupled=False, bias="device")
        p, m, v = (apply_skip(o, n, skip) for o, n in zip((p, m, v), new))
        st["steps"] += 1
        st["good_steps"] += 1
        if st["good_steps"] >= growth_interval:
            scale = scale * torch.tensor(growth, dtype=torch.float32)
            st["good_steps"] = 0
    st["found_inf"] = 0
    st["scale"] = float(scale)
    st["loss_grad"] = float(scale * torch.tensor(base, dtype=torch.float32))
    return p, m, v, st


# ---------------------------------------------------------------- the input recipe
P_SPECIAL = (1e4, -1e4, 1e-20, -0.0)


def optim_inputs(n, gen, *, zero_state=False, tiny_p=False):
    """(p, g, m, v) fp32 [n]: p, g ~ N(0, 1), m ~ 0.1 N(0, 1), v = (0.01 + U(0, 1))^2; then, with k = n // 8,
      [0, k)        g, m x 1e-8 and v x 1e-16: the only place eps = 1e-8 can be seen;
      [k, 2k)       p = 0: the stored parameter is the update itself, not the update rounded at ulp(p);
      2k .. 2k + 3  p = 1e4, -1e4, 1e-20, -0.0;   2k + 4 .. 2k + 7  g = 0   (as far as n reaches).
    ``zero_state``: m = v = 0, the first step.  ``tiny_p``: p of the first block x 1e-8 as well -- the coupled rule adds wd p
    to g and would otherwise swamp the tiny gradients."""
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    m = 0.1 * torch.randn(n, generator=gen, dtype=torch.float64)
    v = (0.01 + torch.rand(n, generator=gen, dtype=torch.float64)) ** 2
    k = n // 8
    g[:k] *= 1e-8
    m[:k] *= 1e-8
    v[:k] *= 1e-16
    if tiny_p:
        p[:k] *= 1e-8
    p[k:2 * k] = 0.0
    for j, x in enumerate(P_SPECIAL):
        if 2 * k + j < n:
            p[2 * k + j] = x
    g[2 * k + 4:2 * k + 8] = 0.0
    if zero_state:
        m.zero_()
        v.zero_()
    return p.float(), g.float(), m.float(), v.float()


def adagrad_inputs(n, gen, *, zero_sum):
    """(p, g, sum) of the recipe with tiny_p; sum is the recipe's v (tiny where g is tiny: eps = 1e-8 shows there) or 0"""
    p, g, _, v = optim_inputs(n, gen, tiny_p=True)
    return p, g, (torch.zeros_like(v) if zero_sum else v)


def skip_mask(n, blocks):
    """uint8 [ceil(n / 64)] with the given 64-blocks set (negative indices count from the last block)"""
    nb = (n + 63) // 64
    s = torch.zeros(nb, dtype=torch.uint8)
    for b in blocks:
        s[b % nb] = 1
    return s
