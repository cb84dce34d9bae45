"""CPU checks of tests/optim_ref.py: the float64 steps equal the torch optimizers they restate, the fp32 chain is inside its
own budget in every regime, and the rule has teeth -- each faulty variant of a step, evaluated in fp32, is rejected where
the tables below say (``ADAM_CAUGHT``, ``SGD_FAULTS``, ``ADAGRAD_FAULTS``).

The tables are the argument that no line of adam_update, sgd_kernel or adagrad_kernel and no pair of hyperparameters at a
call site of csrc/optim.hip can be dropped or exchanged without a named case of tests/test_gpu_optim.py failing: that file
runs every kernel in every regime named here, on these inputs, under this rule."""
import pytest
import torch

from tests import optim_ref as O
from tests.rowwise_ref import fp32_chain

D64 = torch.float64
N = 4099
HYP = dict(lr=5e-3, eps=1e-8, wd=0.09)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- references against the optimizers they restate
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _torch_run(make, p0, grads):
    p = torch.nn.Parameter(p0.clone())
    opt = make([p])
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p.detach(), opt.state[p]


@pytest.mark.parametrize("coupled", [False, True])
def test_adam_step_equals_torch_over_five_steps(coupled):
    g = _gen(1)
    p0 = torch.randn(257, generator=g, dtype=D64)
    grads = [torch.randn(257, generator=g, dtype=D64) for _ in range(5)]
    # values fp32 holds exactly: the reference rounds its hyperparameters to fp32, torch does not
    kw = dict(lr=2.0 ** -7, b1=0.875, b2=0.9375, eps=2.0 ** -27, wd=0.125)
    cls = torch.optim.Adam if coupled else torch.optim.AdamW
    want, state = _torch_run(lambda ps: cls(ps, lr=kw["lr"], betas=(kw["b1"], kw["b2"]), eps=kw["eps"], weight_decay=kw["wd"]),
                             p0, grads)
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for t, gr in enumerate(grads):
        p, m, v = O.adam_step(p, gr, m, v, steps_taken=t, coupled=coupled, bias="device", **kw)
    assert _rel(p, want) < 1e-12 and _rel(m, state["exp_avg"]) < 1e-12 and _rel(v, state["exp_avg_sq"]) < 1e-12
    # the host pair is the device pair rounded to fp32
    ph = O.adam_step(p0, grads[0], torch.zeros_like(p0), torch.zeros_like(p0), steps_taken=0, coupled=coupled, bias="host", **kw)[0]
    pd = O.adam_step(p0, grads[0], torch.zeros_like(p0), torch.zeros_like(p0), steps_taken=0, coupled=coupled, bias="device", **kw)[0]
    assert torch.equal(ph, pd)                                # (1 - b^1 is exact in fp32 for these betas)


@pytest.mark.parametrize("mu,wd", [(0.0, 0.0), (0.0, 0.125), (0.875, 0.0), (0.875, 0.125)])
def test_sgd_step_equals_torch(mu, wd):
    g = _gen(2)
    p0 = torch.randn(129, generator=g, dtype=D64)
    grads = [torch.randn(129, generator=g, dtype=D64) for _ in range(5)]
    want, state = _torch_run(lambda ps: torch.optim.SGD(ps, lr=0.25, momentum=mu, weight_decay=wd), p0, grads)
    p, buf = p0, (torch.zeros_like(p0) if mu else None)       # a zero buffer reproduces torch's "first step: buf = d"
    for gr in grads:
        p, buf = O.sgd_step(p, gr, buf, lr=0.25, mu=mu, wd=wd)
    assert _rel(p, want) < 1e-12
    if mu:
        assert _rel(buf, state["momentum_buffer"]) < 1e-12
    else:
        assert buf is None


@pytest.mark.parametrize("wd", [0.0, 0.125])
def test_adagrad_step_equals_torch(wd):
    """clr is rounded to fp32, as the kernel's launcher rounds it, and lr / (1 + (t - 1) lr_decay) is not an fp32 number at
    every one of five steps whatever lr_decay != 0 is chosen.  So: to 1e-12 against torch.optim.Adagrad handed that rounded
    clr at every step, clr itself against torch's formula, and against torch's own lr_decay within the rounding of clr."""
    g = _gen(3)
    p0 = torch.randn(129, generator=g, dtype=D64)
    grads = [torch.randn(129, generator=g, dtype=D64) for _ in range(5)]
    kw = dict(lr=0.25, lr_decay=0.125, eps=2.0 ** -30, wd=wd)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adagrad([pt], lr=0.25, lr_decay=0.0, eps=kw["eps"], weight_decay=wd)
    p, s = p0, torch.zeros_like(p0)
    for t, gr in enumerate(grads):
        p, s = O.adagrad_step(p, gr, s, step=t + 1, **kw)
        opt.param_groups[0]["lr"] = O.adagrad_clr(0.25, 0.125, t + 1)
        pt.grad = gr.clone()
        opt.step()
        assert O.adagrad_clr(0.25, 0.125, t + 1) == O.f32(0.25 / (1 + t * 0.125))
    assert _rel(p, pt.detach()) < 1e-12 and _rel(s, opt.state[pt]["sum"]) < 1e-12
    want, state = _torch_run(lambda ps: torch.optim.Adagrad(ps, lr=0.25, lr_decay=0.125, eps=kw["eps"], weight_decay=wd), p0, grads)
    assert float((p - want).abs().max()) < 5 * 0.25 * 2.0 ** -24 and _rel(s, state["sum"]) < 1e-8
    assert O.adagrad_clr(0.25, 0.125, 1) == 0.25 and O.adagrad_clr(0.25, 0.125, 9) == 0.125


def test_scaled_step_follows_gradscaler_on_a_scripted_sequence():
    """clean, overflow, clean, clean at growth_interval 2: torch.amp.GradScaler's scale after every update()"""
    gen = _gen(4)
    p, g, m, v = (t.double() for t in O.optim_inputs(130, gen))
    kw = dict(lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.09, growth_interval=2, growth=2.0, backoff=0.5, base=0.25)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    st = O.scaler_state(1024.0)
    steps = 0
    for k, bad in enumerate([False, True, False, False]):
        gk = g * st["scale"]
        if bad:
            gk = gk.clone()
            gk[77] = float("inf")
        # GradScaler's own rule, driven the way its step() / update() drive it
        found = torch.tensor([1.0 if bad else 0.0])
        scaler._scale = torch.tensor(st["scale"]) if scaler._scale is None else scaler._scale
        scaler._growth_tracker = torch.zeros(1, dtype=torch.int32) if scaler._growth_tracker is None else scaler._growth_tracker
        torch._amp_update_scale_(scaler._scale, scaler._growth_tracker, found, 2.0, 0.5, 2)
        before = (p, m, v)
        p, m, v, st = O.scaled_step(p, gk, m, v, st, **kw)
        steps += 0 if bad else 1
        assert st["scale"] == float(scaler._scale) and st["good_steps"] == int(scaler._growth_tracker), k
        assert st["steps"] == steps and st["found_inf"] == 0 and st["loss_grad"] == st["scale"] * 0.25
        if bad:
            assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v)))
        else:
            want = O.adam_step(*before[:1], g, *before[1:], lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.09,
                               steps_taken=steps - 1, coupled=False, bias="device")
            assert all(torch.equal(a, b) for a, b in zip(want, (p, m, v)))      # a power-of-two scale divides out exactly
    assert [st["scale"], st["good_steps"], st["steps"]] == [1024.0, 0, 3]       # halved once, doubled once


def test_scaled_step_skips_on_an_inf_inside_a_skipped_block():
    p, g, m, v = (t.double() for t in O.optim_inputs(200, _gen(5)))
    skip = O.skip_mask(200, [1])
    g[70] = float("-inf")
    kw = dict(lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.09, growth_interval=2, growth=2.0, backoff=0.5, base=1.0)
    p2, m2, v2, st = O.scaled_step(p, g, m, v, O.scaler_state(8.0), skip=skip, **kw)
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v) and st["scale"] == 4.0 and st["steps"] == 0
    g[70] = 3.4028234663852886e38                              # the largest float is not an overflow
    p2, m2, v2, st = O.scaled_step(p, g, m, v, O.scaler_state(8.0), skip=skip, **kw)
    assert st["scale"] == 8.0 and st["steps"] == 1 and st["good_steps"] == 1
    assert torch.equal(p2[64:128], p[64:128]) and not torch.equal(p2[:64], p[:64]) and not torch.equal(v2[128:], v[128:])


def test_apply_skip_and_inputs():
    old, new = torch.zeros(130), torch.ones(130)
    out = O.apply_skip(old, new, O.skip_mask(130, [0, -1]))
    assert out[:64].sum() == 0 and out[64:128].sum() == 64 and out[128:].sum() == 0          # the last block is partial
    assert O.apply_skip(old, new, None) is new
    assert O.skip_mask(4099, [-1]).numel() == 65 and int(O.skip_mask(4099, [-1])[64]) == 1
    a, b = O.optim_inputs(N, _gen(7), tiny_p=True), O.optim_inputs(N, _gen(7), tiny_p=True)
    assert all(torch.equal(x, y) and x.dtype == torch.float32 for x, y in zip(a, b))
    assert not torch.equal(a[0], O.optim_inputs(N, _gen(8), tiny_p=True)[0])
    p, g, m, v = O.optim_inputs(N, _gen(7))
    k = N // 8
    assert float(g[:k].abs().max()) < 1e-7 and float(v[:k].max()) < 2e-16 and float(p[:k].abs().max()) > 1
    assert float(a[0][:k].abs().max()) < 1e-7 and not p[k:2 * k].any() and p[2 * k:2 * k + 4].tolist()[:2] == [1e4, -1e4]
    assert float(p[2 * k + 2]) == pytest.approx(1e-20) and torch.signbit(p[2 * k + 3]) and not g[2 * k + 4:2 * k + 8].any()
    assert float(v.min()) > 0
    z = O.optim_inputs(N, _gen(7), zero_state=True)
    assert not z[2].any() and not z[3].any() and torch.equal(z[1], g)
    for n in (1, 3, 4, 5):                                   # the recipe holds at the sizes below one block of specials
        assert all(t.numel() == n and bool(torch.isfinite(t).all()) for t in O.optim_inputs(n, _gen(n)))


# ---------------------------------------------------------------- the chain inside its own budget; the faulty variants outside
def _hyper(regime, coupled):
    b1, b2, t, K = O.REGIMES[regime]
    return dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=coupled, bias="device"), K


@pytest.mark.parametrize("coupled", [False, True], ids=["adamw", "adam"])
@pytest.mark.parametrize("regime", list(O.REGIMES))
def test_the_fp32_chain_is_inside_the_budget(regime, coupled):
    hyper, K = _hyper(regime, coupled)
    for zero_state in (False, True):
        inputs = O.optim_inputs(N, _gen(11), zero_state=zero_state, tiny_p=coupled)
        for bias in ("device", "host"):
            h = dict(hyper, bias=bias)
            r = O.check_adam(fp32_chain(O.adam_step, *inputs, **h), inputs, h, K=K if bias == "device" else None, what=regime)
            assert max(r.values()) <= 0.25 + 1e-9, r          # the chain is the w of E = (4 w + 1) ulp


def faulty_adam(p, g, m, v, *, fault, lr, b1, b2, eps, wd, steps_taken, coupled, bias):
    """``optim_ref.adam_step`` with one fault"""
    if fault == "t_off_by_one":
        steps_taken += 1
    if fault == "decay_swapped":
        coupled = not coupled
    bc1, bc2s = O.bias_pair(b1, b2, steps_taken, p.dtype, bias)
    if fault == "no_bias_correction_of_v":
        bc2s = torch.ones_like(bc2s)
    lr, b1, b2, eps, wd = O._scalars(p, lr, b1, b2, eps, wd)
    step_size = lr / bc1
    p0 = p
    if coupled:
        g = g + wd * p
    elif fault != "decay_after_update":
        p = p * (1 - lr * wd)
    m = (b2 * m + (1 - b2) * g) if fault == "betas_exchanged_in_m" else (b1 * m + (1 - b1) * g)
    v = b2 * v + (1 - b2) * (g if fault == "g_not_squared" else g * g)
    den = ((v.sqrt() + eps) / bc2s) if fault == "eps_inside_the_root_correction" else (v.sqrt() / bc2s + eps)
    p = p - step_size * (m / den)
    if fault == "decay_after_update" and not coupled:
        p = p * (1 - lr * wd)
    return p, m, v


# fault -> the regimes in which the rule rejects it on p, m or v, for AdamW and for the coupled rule (inputs with tiny_p).
# The three bias-correction faults are not seen once the powers are negligible: that is why the other regimes exist.
_ALL = set(O.REGIMES)
_EARLY = {r for r in O.REGIMES if not r.startswith("negligible")}
ADAM_CAUGHT = {
    "eps_inside_the_root_correction": (_EARLY, _EARLY),
    "decay_swapped": (_ALL, _ALL),
    "decay_after_update": (_ALL - {"workload-0"}, None),       # (the coupled rule has no decay factor to misplace)
    "t_off_by_one": (_EARLY, _EARLY),
    "betas_exchanged_in_m": (_ALL, _ALL),
    "g_not_squared": (_ALL, _ALL),
    "no_bias_correction_of_v": (_EARLY, _EARLY),
}


def _rejected(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("coupled", [False, True], ids=["adamw", "adam"])
@pytest.mark.parametrize("fault", list(ADAM_CAUGHT))
def test_every_adam_fault_is_rejected_where_the_table_says(fault, coupled):
    want = ADAM_CAUGHT[fault][coupled]
    if want is None:
        return
    caught = set()
    for regime in O.REGIMES:
        hyper, K = _hyper(regime, coupled)
        inputs = O.optim_inputs(N, _gen(11), tiny_p=coupled)
        got = tuple(t.float() for t in faulty_adam(*inputs, fault=fault, **hyper))
        if _rejected(O.check_adam, got, inputs, hyper, K=K, what=f"{fault} {regime}"):
            caught.add(regime)
    assert caught == want, (fault, sorted(caught), sorted(want))
    assert caught, fault


@pytest.mark.parametrize("coupled", [False, True], ids=["adamw", "adam"])
def test_every_exchange_of_two_hyperparameters_is_rejected(coupled):
    """two floats exchanged at a call site of csrc/optim.hip: seen in every regime (the first and the last are taken)"""
    import itertools
    inputs = O.optim_inputs(N, _gen(11), tiny_p=coupled)
    for regime in ("negligible-29999", "workload-0"):
        hyper, K = _hyper(regime, coupled)
        for a, b in itertools.combinations(("lr", "b1", "b2", "eps", "wd"), 2):
            swapped = dict(hyper, **{a: hyper[b], b: hyper[a]})
            got = fp32_chain(O.adam_step, *inputs, **swapped)
            assert _rejected(O.check_adam, got, inputs, hyper, K=K), (regime, a, b)


def faulty_sgd(p, g, buf, *, fault, lr, mu, wd):
    lr_, mu_, wd_ = O._scalars(p, lr, mu, wd)
    d = g if fault == "wd_ignored" else g + wd_ * p
    if O.f32(mu) == 0.0:
        return p - lr_ * d, (d if fault == "buf_written_without_momentum" else buf)
    if fault == "lr_and_mu_exchanged":
        lr_, mu_ = mu_, lr_
    buf = (buf + mu_ * d) if fault == "momentum_on_d" else (mu_ * buf + d)
    return p - lr_ * buf, buf


# fault -> the (mu, wd) of tests/test_gpu_optim.py's SGD cases that reject it, with a non-zero buffer
SGD_CASES = [(mu, wd) for mu in (0.0, 0.005, 0.9) for wd in (0.0, 0.09)]
SGD_FAULTS = {
    "momentum_on_d": {(0.005, 0.0), (0.005, 0.09), (0.9, 0.0), (0.9, 0.09)},
    "buf_written_without_momentum": {(0.0, 0.0), (0.0, 0.09)},
    "wd_ignored": {(0.0, 0.09), (0.005, 0.09), (0.9, 0.09)},
    "lr_and_mu_exchanged": {(0.005, 0.0), (0.005, 0.09), (0.9, 0.0), (0.9, 0.09)},
}


@pytest.mark.parametrize("fault", list(SGD_FAULTS))
def test_every_sgd_fault_is_rejected_where_the_table_says(fault):
    caught = set()
    p, g, buf, _ = O.optim_inputs(N, _gen(12))
    for mu, wd in SGD_CASES:
        hyper = dict(lr=0.05, mu=mu, wd=wd)
        gp, gb = faulty_sgd(p, g, buf, fault=fault, **hyper)
        bad = _rejected(O.check_sgd, (gp, gb), (p, g, buf), hyper)
        if mu == 0.0 and not torch.equal(gb, buf):           # the buffer of a momentum-free step: untouched, bit for bit
            bad = True
        if bad:
            caught.add((mu, wd))
    assert caught == SGD_FAULTS[fault], (fault, sorted(caught))


def faulty_adagrad(p, g, s, *, fault, lr, lr_decay, eps, wd, step):
    clr, eps_, wd_ = O._scalars(p, O.adagrad_clr(lr, 0.0 if fault == "lr_decay_ignored" else lr_decay, step), eps, wd)
    d = g if fault == "wd_ignored" else g + wd_ * p
    s = s + d * d
    den = (s + eps_).sqrt() if fault == "eps_inside_the_root" else s.sqrt() + eps_
    return p - clr * (d / den), s


ADAGRAD_CASES = [(step, dec, wd) for step in (1, 7) for dec in (0.0, 0.1) for wd in (0.0, 0.09)]
ADAGRAD_FAULTS = {
    "wd_ignored": {c for c in ADAGRAD_CASES if c[2] != 0.0},
    "eps_inside_the_root": set(ADAGRAD_CASES),
    "lr_decay_ignored": {c for c in ADAGRAD_CASES if c[0] == 7 and c[1] != 0.0},
}

@pytest.mark.parametrize("fault", list(ADAGRAD_FAULTS))
def test_every_adagrad_fault_is_rejected_where_the_table_says(fault):
    caught = set()
    inputs = O.adagrad_inputs(N, _gen(13), zero_sum=False)
    for step, dec, wd in ADAGRAD_CASES:
        hyper = dict(lr=0.05, lr_decay=dec, eps=1e-8, wd=wd, step=step)
        got = faulty_adagrad(*inputs, fault=fault, **hyper)
        assert not _rejected(O.check_adagrad, O.adagrad_step(*inputs, **hyper), inputs, hyper)
        if _rejected(O.check_adagrad, got, inputs, hyper):
            caught.add((step, dec, wd))
    assert caught == ADAGRAD_FAULTS[fault], (fault, sorted(caught))


def test_the_sgd_chain_is_inside_the_budget():
    p, g, buf, _ = O.optim_inputs(N, _gen(12))
    for mu, wd in SGD_CASES:
        for b in (buf, torch.zeros_like(buf)):
            hyper = dict(lr=0.05, mu=mu, wd=wd)
            r = O.check_sgd(O.sgd_step(p, g, b, **hyper), (p, g, b), hyper)
            assert max(r.values()) <= 0.25 + 1e-9, r
