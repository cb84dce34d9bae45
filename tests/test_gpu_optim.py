"""The streaming optimizer kernels of csrc/optim.hip called directly through ops.*, each after ONE launch from a handed
state against the float64 statement of tests/optim_ref.py under that file's tolerance rule (its docstring has the rule,
the three regimes of the device-side bias correction and where K = 16 comes from).  A second consecutive launch starts
from the GPU's own state read back, which is handed to the reference: nothing is compared after a trajectory.

Every p, g, state and mirror tensor handed over is the middle of a larger NaN-filled buffer (``Held``): the bands of 64
elements before and after must still be NaN afterwards, and g must be unchanged bit for bit.  A 16-bit mirror must equal
the fp32 parameter the same launch wrote, cast to the dtype, bit for bit -- skipped blocks and the n % 4 tail included.

Each case prints its worst error as a fraction of the budget (``[optim] ...``; run with -s to collect them).  Measured on
an MI355X, the worst over all cases of a regime: powers negligible 0.23, powers small 0.82 (exp_avg in
test_adam_step_dev_misaligned, whose four sizes end at 1027; 0.33 in every other case), workload betas 0.27 -- the chain
itself sits at 0.25 or below by construction.  SGD 0.26, Adagrad 0.32, the loss-scaled step 0.24."""
import math

import pytest
import torch

from tests import optim_ref as O

pytestmark = pytest.mark.gpu

GUARD = 64
NS = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1027, 4099]      # n & 3 = 0..3; a part workgroup, a whole one; 64-block edges
N_SCALAR_TRIPS = (1 << 20) + (1 << 17) + 67              # past 8 x CUs x 256 threads, and past adam_dev_kernel's 4096 x 256
N_FUSED_TRIPS = 5 * (1 << 19) + 67                       # its quads past 8 x CUs x 256 threads
HYP = dict(lr=5e-3, eps=1e-8, wd=0.09)
MIRRORS = {"none": None, "bf16": torch.bfloat16, "fp16": torch.float16}
REGIME_IDS = list(O.REGIMES)


@pytest.fixture(scope="module")
def ops(device):
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd.ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Held:
    """a tensor handed to a kernel as the middle of a larger NaN-filled device buffer, ``offset`` elements further in"""

    def __init__(self, src, device, offset=0):
        self.n, self.lo = src.numel(), GUARD + offset
        self.buf = torch.full((self.n + 2 * GUARD + offset,), math.nan, dtype=src.dtype, device=device)
        self.t = self.buf[self.lo:self.lo + self.n]
        self.t.copy_(src)

    def cpu(self):
        return self.t.cpu()

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


def _hold(device, *tensors, offset=0):
    return [Held(t, device, offset) for t in tensors]


def _mirror(n, dtype, device, offset=0):
    return None if dtype is None else Held(torch.full((n,), math.nan, dtype=dtype), device, offset)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _kw(h):
    return dict(beta1=h["b1"], beta2=h["b2"], eps=h["eps"], weight_decay=h["wd"])


def _skip_for(n):
    """the first, a middle and the last 64-block set (the last is partial when n % 64 != 0); below four blocks the last"""
    nb = (n + 63) // 64
    return O.skip_mask(n, [0, nb // 2, -1] if nb >= 4 else [-1])


def _after(held, g, olds, skip, mirror=None, what=""):
    """what every launch must leave: the bands, g, the skipped blocks and the mirror; -> the state tensors on the CPU"""
    got = [h.cpu() for h in held]
    assert all(h.intact() for h in held), f"{what}: a guard band was written"
    assert _same_bits(got[1], g), f"{what}: the gradient was written"
    got = [got[0]] + got[2:]
    if skip is not None:
        mask = skip.bool().repeat_interleave(64)[:g.numel()]
        for gt, old in zip(got, olds):
            assert _same_bits(gt[mask], old[mask]), f"{what}: a skipped block was written"
    if mirror is not None:
        assert mirror.intact(), f"{what}: a guard band of the mirror was written"
        assert _same_bits(mirror.cpu(), got[0].to(mirror.t.dtype)), f"{what}: the mirror is not the parameter cast"
    return got


def _report(what, r):
    print(f"[optim] {what}: worst error / budget " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))


def _worse(a, b):
    return b if a is None else {k: max(a[k], b[k]) for k in b}


# ---------------------------------------------------------------- AdamW, bias correction from the host
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
@pytest.mark.parametrize("betas", ["workload", "small"])
def test_adamw_step(ops, device, betas, step):
    b1, b2 = (0.9, 0.999) if betas == "workload" else (2.0 ** -4, 2.0 ** -5)
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=step - 1, coupled=False, bias="host")
    worst = None
    for n in NS:
        for zero_state in ((False, True) if step == 1 else (False,)):
            p, g, m, v = O.optim_inputs(n, _gen(n), zero_state=zero_state)
            held = _hold(device, p, g, m, v)
            ops.adamw_step_(*(h.t for h in held), lr=hyper["lr"], step=step, **_kw(hyper))
            what = f"adamw_step_ {betas} step={step} n={n} zero_state={zero_state}"
            got = _after(held, g, (p, m, v), None, what=what)
            worst = _worse(worst, O.check_adam(got, (p, g, m, v), hyper, what=what))     # never the scalar term
    _report(f"adamw_step_ {betas} step={step}", worst)


# ---------------------------------------------------------------- AdamW, counter on the device
@pytest.mark.parametrize("skipped", [False, True], ids=["all", "skip"])
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_adamw_step_dev(ops, device, regime, skipped):
    b1, b2, t, K = O.REGIMES[regime]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=False, bias="device")
    worst = None
    for n in NS:
        p, g, m, v = O.optim_inputs(n, _gen(100 + n), zero_state=(t == 0))
        skip = _skip_for(n) if skipped else None
        held = _hold(device, p, g, m, v)
        counter = torch.tensor([t], dtype=torch.int64, device=device)
        ops.adamw_step_dev_(*(h.t for h in held), counter, lr=hyper["lr"], skip=None if skip is None else skip.to(device),
                            **_kw(hyper))
        what = f"adamw_step_dev_ {regime} n={n} skip={skipped}"
        assert counter.tolist() == [t + 1], what
        got = _after(held, g, (p, m, v), skip, what=what)
        worst = _worse(worst, O.check_adam(got, (p, g, m, v), hyper, K=K, skip=skip, what=what))
    _report(f"adamw_step_dev_ {regime} skip={skipped}", worst)


# ---------------------------------------------------------------- the two one-launch steps with mirror and ticket
def _two_launches(launch, device, n, t, hyper, K, mirror_dtype, *, tiny_p, seed, offset=0, what=""):
    """launch 1 from the recipe at ``t`` steps taken, every block; launch 2 from the state launch 1 left (read back and
    handed to the reference), with the skip mask.  -> the worse of the two results"""
    p, g, m, v = O.optim_inputs(n, _gen(seed), zero_state=(t == 0), tiny_p=tiny_p)
    held = _hold(device, p, g, m, v, offset=offset)
    mirror = _mirror(n, mirror_dtype, device, offset)
    counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
    worst = None
    for k, skip in enumerate((None, _skip_for(n))):
        h = dict(hyper, steps_taken=t + k)
        launch(held, counter, None if skip is None else skip.to(device), None if mirror is None else mirror.t)
        tag = f"{what} n={n} launch {k + 1}"
        assert counter.tolist() == [t + k + 1, 0], f"{tag}: the counter is published once, the ticket is back at 0"
        got = _after(held, g, (p, m, v), skip, mirror, what=tag)
        worst = _worse(worst, O.check_adam(got, (p, g, m, v), h, K=K, skip=skip, what=tag))
        p, m, v = got
    return worst


@pytest.mark.parametrize("regime", REGIME_IDS)
@pytest.mark.parametrize("mirror", list(MIRRORS))
def test_adamw_step_fused(ops, device, mirror, regime):
    b1, b2, t, K = O.REGIMES[regime]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=False, bias="device")

    def launch(held, counter, skip, mir):
        ops.adamw_step_fused_(*(h.t for h in held), counter, lr=hyper["lr"], skip=skip, mirror=mir, **_kw(hyper))
    worst = None
    for n in NS:
        worst = _worse(worst, _two_launches(launch, device, n, t, hyper, K, MIRRORS[mirror], tiny_p=False, seed=200 + n,
                                            what=f"adamw_step_fused_ {mirror} {regime}"))
    _report(f"adamw_step_fused_ {mirror} {regime}", worst)


def test_adamw_step_fused_alignment(ops, device):
    """an offset of 4 floats (16 bytes) is accepted; an offset of 1 float is refused with DVT_REQUIRE's message and nothing
    is written"""
    b1, b2, t, K = O.REGIMES["negligible-29999"]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=False, bias="device")

    def launch(held, counter, skip, mir):
        ops.adamw_step_fused_(*(h.t for h in held), counter, lr=hyper["lr"], skip=skip, mirror=mir, **_kw(hyper))
    for n in (5, 1027):
        _report(f"adamw_step_fused_ offset 4 n={n}", _two_launches(launch, device, n, t, hyper, K, torch.bfloat16, tiny_p=False,
                                                                    seed=n, offset=4, what="adamw_step_fused_ offset 4"))
        p, g, m, v = O.optim_inputs(n, _gen(n))
        for off in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
            held = [Held(x, device, o) for x, o in zip((p, g, m, v), off)]
            counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
            with pytest.raises(RuntimeError, match="dvt_adamw_step_fused: buffers must be 16-byte aligned"):
                launch(held, counter, None, None)
            torch.cuda.synchronize()
            assert counter.tolist() == [t, 0] and all(h.intact() for h in held)
            assert all(_same_bits(h.cpu(), x) for h, x in zip(held, (p, g, m, v))), off


def _adam_dev_launch(ops, hyper, lr_dev):
    def launch(held, counter, skip, mir):
        ops.adam_step_dev_(*(h.t for h in held), counter, lr_dev, skip=skip, mirror=mir, **_kw(hyper))
    return launch


@pytest.mark.parametrize("regime", REGIME_IDS)
@pytest.mark.parametrize("mirror", list(MIRRORS))
def test_adam_step_dev(ops, device, mirror, regime):
    """torch.optim.Adam's coupled decay, the rate read from the device; inputs with tiny_p"""
    b1, b2, t, K = O.REGIMES[regime]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=True, bias="device")
    lr_dev = torch.tensor([hyper["lr"]], dtype=torch.float32, device=device)
    worst = None
    for n in NS:
        worst = _worse(worst, _two_launches(_adam_dev_launch(ops, hyper, lr_dev), device, n, t, hyper, K, MIRRORS[mirror],
                                            tiny_p=True, seed=300 + n, what=f"adam_step_dev_ {mirror} {regime}"))
    _report(f"adam_step_dev_ {mirror} {regime}", worst)


@pytest.mark.parametrize("mirror", list(MIRRORS))
def test_adam_step_dev_misaligned(ops, device, mirror):
    """the kernel is scalar: p, g, m, v one float and the mirror one element off 16-byte alignment are accepted"""
    b1, b2, t, K = O.REGIMES["small-1"]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=True, bias="device")
    lr_dev = torch.tensor([hyper["lr"]], dtype=torch.float32, device=device)
    probe = Held(torch.zeros(4), device, 1)
    assert probe.t.data_ptr() % 16 == 4
    if MIRRORS[mirror] is not None:
        assert _mirror(4, MIRRORS[mirror], device, 1).t.data_ptr() % 4 == 2
    worst = None
    for n in (1, 5, 65, 1027):
        worst = _worse(worst, _two_launches(_adam_dev_launch(ops, hyper, lr_dev), device, n, t, hyper, K, MIRRORS[mirror],
                                            tiny_p=True, seed=400 + n, offset=1, what=f"adam_step_dev_ misaligned {mirror}"))
    _report(f"adam_step_dev_ misaligned {mirror}", worst)


def test_adam_step_dev_zero_rate(ops, device):
    """lr = 0 on the device: p bit-equal (-0.0 and 1e-20 included), the moments moved as the rule says"""
    b1, b2, t, K = O.REGIMES["workload-1"]
    hyper = dict(HYP, lr=0.0, b1=b1, b2=b2, steps_taken=t, coupled=True, bias="device")
    lr_dev = torch.zeros(1, dtype=torch.float32, device=device)
    for n in (5, 257, 4099):
        p, g, m, v = O.optim_inputs(n, _gen(500 + n), tiny_p=True)
        held = _hold(device, p, g, m, v)
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        _adam_dev_launch(ops, hyper, lr_dev)(held, counter, None, None)
        assert counter.tolist() == [t + 1, 0]
        got = _after(held, g, (p, m, v), None, what=f"lr=0 n={n}")
        assert torch.equal(got[0], p) and not torch.equal(got[1], m) and not torch.equal(got[2], v)
        O.check_adam(got, (p, g, m, v), hyper, K=K, what=f"adam_step_dev_ lr=0 n={n}")


# ---------------------------------------------------------------- SGD, Adagrad
@pytest.mark.parametrize("wd", [0.0, 0.09])
@pytest.mark.parametrize("mu", [0.0, 0.005, 0.9])
def test_sgd_step(ops, device, mu, wd):
    hyper = dict(lr=0.05, mu=mu, wd=wd)
    worst = None
    for n in NS:
        p, g, buf, _ = O.optim_inputs(n, _gen(600 + n))
        for b in (buf, torch.zeros_like(buf)):               # a later step; the first
            for skip in (None, _skip_for(n)):
                held = _hold(device, p, g, b)
                ops.sgd_step_(*(h.t for h in held), lr=0.05, momentum=mu, weight_decay=wd,
                              skip=None if skip is None else skip.to(device))
                what = f"sgd_step_ mu={mu} wd={wd} n={n} skip={skip is not None}"
                got = _after(held, g, (p, b), skip, what=what)
                if mu == 0.0:
                    assert _same_bits(got[1], b), f"{what}: the buffer of a momentum-free step was written"
                worst = _worse(worst, O.check_sgd(got, (p, g, b), hyper, skip=skip, what=what))
        if mu == 0.0:
            held = _hold(device, p, g)                        # no buffer at all
            ops.sgd_step_(held[0].t, held[1].t, None, lr=0.05, momentum=0.0, weight_decay=wd)
            got = _after(held, g, (p,), None, what=f"sgd_step_ no buffer n={n}")
            O.check_sgd((got[0], None), (p, g, None), hyper, what=f"sgd_step_ no buffer n={n}")
            held = _hold(device, p, g, torch.full_like(p, math.nan))      # a poisoned one: stays as it is
            ops.sgd_step_(*(h.t for h in held), lr=0.05, momentum=0.0, weight_decay=wd)
            assert bool(torch.isnan(held[2].buf).all()) and _same_bits(held[0].cpu(), got[0])
    _report(f"sgd_step_ mu={mu} wd={wd}", worst)


@pytest.mark.parametrize("wd", [0.0, 0.09])
@pytest.mark.parametrize("lr_decay", [0.0, 0.1])
@pytest.mark.parametrize("step", [1, 7])
def test_adagrad_step(ops, device, step, lr_decay, wd):
    hyper = dict(lr=0.05, lr_decay=lr_decay, eps=1e-8, wd=wd, step=step)
    worst = None
    for n in NS:
        for zero_sum in (False, True):
            p, g, s = O.adagrad_inputs(n, _gen(700 + n), zero_sum=zero_sum)
            for skip in (None, _skip_for(n)):
                held = _hold(device, p, g, s)
                ops.adagrad_step_(*(h.t for h in held), skip=None if skip is None else skip.to(device), lr=0.05,
                                  lr_decay=lr_decay, eps=1e-8, weight_decay=wd, step=step)
                what = f"adagrad_step_ step={step} lr_decay={lr_decay} wd={wd} n={n} zero_sum={zero_sum} skip={skip is not None}"
                got = _after(held, g, (p, s), skip, what=what)
                worst = _worse(worst, O.check_adagrad(got, (p, g, s), hyper, skip=skip, what=what))
                if zero_sum and wd == 0.0:                    # g = 0 on sum = 0: 0 / (0 + eps), p as it was, not NaN
                    still = g == 0
                    assert _same_bits(got[0][still], p[still]) and not got[1][still].any(), what
    _report(f"adagrad_step_ step={step} lr_decay={lr_decay} wd={wd}", worst)


# ---------------------------------------------------------------- AdamW under loss scaling: the state machine
SCALED = dict(lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.09, growth_interval=2, growth=2.0, backoff=0.5, base=0.25)


class _Scaler:
    """the device state of ops.adamw_step_scaled_"""

    def __init__(self, st, device):
        self.step = torch.tensor([st["steps"]], dtype=torch.int64, device=device)
        self.scale = torch.tensor([st["scale"]], dtype=torch.float32, device=device)
        self.found = torch.tensor([st["found_inf"]], dtype=torch.int32, device=device)
        self.good = torch.tensor([st["good_steps"]], dtype=torch.int32, device=device)
        self.loss_grad = torch.full((1,), math.nan, dtype=torch.float32, device=device)

    def args(self):
        return self.step, self.scale, self.found, self.good, self.loss_grad

    def state(self):
        return dict(steps=int(self.step), scale=float(self.scale), found_inf=int(self.found), good_steps=int(self.good),
                    loss_grad=float(self.loss_grad))


def _scaled_launch(ops, held, sc, skip, kw=SCALED):
    ops.adamw_step_scaled_(*(h.t for h in held), *sc.args(), lr=kw["lr"], beta1=kw["b1"], beta2=kw["b2"], eps=kw["eps"],
                           weight_decay=kw["wd"], growth_interval=kw["growth_interval"], growth=kw["growth"],
                           backoff=kw["backoff"], loss_grad_base=kw["base"], skip=skip)


def _bad_gradient(g, kind, skip):
    n = g.numel()
    g = g.clone()
    if kind == "inf-first":
        g[0] = math.inf
    elif kind == "neginf-last":
        g[n - 1] = -math.inf
    elif kind == "nan-middle":
        g[n // 2] = math.nan
    else:                                                    # inside a skipped block: the whole step is skipped all the same
        i = int(skip.nonzero()[0]) * 64 + 1
        assert i < n
        g[i] = math.inf
    return g


@pytest.mark.parametrize("start", [0, 29999])
@pytest.mark.parametrize("kind", ["inf-first", "neginf-last", "nan-middle", "inf-skipped"])
def test_adamw_step_scaled(ops, device, kind, start):
    """five launches on one buffer: clean, overflow, clean, clean (the scale grows at growth_interval = 2), overflow.
    The contract for a non-finite value inside a skipped block: check_finite_kernel reads the whole gradient, so the step
    is skipped as a whole and the scale backs off -- the mask says which parameters have a gradient, not which gradient
    values count."""
    K = O.POWF_ULPS if start == 0 else None
    for n in (65, 4099):
        p, g0, m, v = O.optim_inputs(n, _gen(800 + n), zero_state=(start == 0))
        skip = O.skip_mask(n, [(n + 63) // 64 // 2 + 1]) if kind == "inf-skipped" else None
        st = O.scaler_state(1024.0, steps=start)
        sc = _Scaler(st, device)
        held = _hold(device, p, g0, m, v)
        for k, bad in enumerate([False, True, False, False, True]):
            g = g0 * st["scale"]                              # a power of two: exact
            if bad:
                g = _bad_gradient(g, kind, skip)
            held[1].t.copy_(g)
            _scaled_launch(ops, held, sc, None if skip is None else skip.to(device))
            what = f"adamw_step_scaled_ {kind} start={start} n={n} launch {k + 1}"
            got = _after(held, g, (p, m, v), skip, what=what)
            hyper = dict(HYP, b1=0.9, b2=0.999, steps_taken=st["steps"], coupled=False, bias="device")
            rp, rm, rv, st = O.scaled_step(p, g, m, v, st, skip=skip, **SCALED)
            assert sc.state() == st, f"{what}: {sc.state()} != {st}"
            if bad:
                assert all(_same_bits(a, b) for a, b in zip(got, (p, m, v))), f"{what}: an overflowed step moved something"
            else:
                assert all(_same_bits(a, b) for a, b in zip((rp, rm, rv), fp_chain_of_scaled(p, g0, m, v, hyper, skip)))
                r = O.check_adam(got, (p, g0, m, v), hyper, K=K, skip=skip, what=what)
                if k == 0:
                    _report(what, r)
            p, m, v = got
        assert st["steps"] == start + 3 and st["scale"] == 512.0 and st["good_steps"] == 0      # /2, x2, /2


def fp_chain_of_scaled(p, g0, m, v, hyper, skip):
    """scaled_step on scale * g0 is adam_step on g0 (the scale is a power of two): the rule is applied to g / scale"""
    new = O.adam_step(p, g0, m, v, **hyper)
    return tuple(O.apply_skip(o, x, skip) for o, x in zip((p, m, v), new))


def test_adamw_step_scaled_largest_float_is_no_overflow(ops, device):
    n = 257
    p, g0, m, v = O.optim_inputs(n, _gen(900))
    kw = dict(SCALED, growth_interval=1000)
    st = O.scaler_state(2.0 ** 100, steps=29999)
    g = g0 * st["scale"]
    g[0], g[n - 1] = 3.4028234663852886e38, -3.4028234663852886e38
    sc = _Scaler(st, device)
    held = _hold(device, p, g, m, v)
    _scaled_launch(ops, held, sc, None, kw)
    got = _after(held, g, (p, m, v), None, what="largest float")
    _, _, _, st = O.scaled_step(p, g, m, v, st, **kw)
    assert sc.state() == st and st["steps"] == 30000 and st["scale"] == 2.0 ** 100 and st["good_steps"] == 1
    hyper = dict(HYP, b1=0.9, b2=0.999, steps_taken=29999, coupled=False, bias="device")
    O.check_adam(got, (p, g / 2.0 ** 100, m, v), hyper, what="adamw_step_scaled_ largest float")


def test_adamw_step_scaled_empty(ops, device):
    """n = 0 the way ops hands it over (empty tensors carry null pointers): only the scaler state moves, as after a clean step"""
    held = _hold(device, *(torch.zeros(0) for _ in range(4)))
    st = O.scaler_state(1024.0, steps=5, good_steps=1)
    sc = _Scaler(st, device)
    _scaled_launch(ops, held, sc, None)
    assert all(h.intact() for h in held)
    empty = torch.zeros(0)
    _, _, _, st = O.scaled_step(empty, empty, empty, empty, st, **SCALED)
    assert sc.state() == st and st == dict(steps=6, scale=2048.0, found_inf=0, good_steps=0, loss_grad=512.0)


# ---------------------------------------------------------------- later trips of the grid-stride loops
def _trip_case(device, n, per_thread, tiny_p=False):
    """inputs at ``n``, a skip mask with one block set beyond the first trip, and the proof that ``n`` wraps the grid"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first_trip = 256 * 8 * cus * per_thread                  # elements the capped grid covers in one trip
    assert n > first_trip, f"n = {n} does not exceed the grid of {cus} CUs ({first_trip} elements per trip)"
    block = (n - 200) >> 6
    assert block * 64 >= first_trip
    b1, b2, t, K = O.REGIMES["negligible-29999"]
    hyper = dict(HYP, b1=b1, b2=b2, steps_taken=t, coupled=tiny_p, bias="device")
    return O.optim_inputs(n, _gen(n), tiny_p=tiny_p), O.skip_mask(n, [block]), hyper, t


TRIPS = ["adamw_step_", "adamw_step_dev_", "adamw_step_fused_-none", "adamw_step_fused_-bf16", "adam_step_dev_-none",
         "adam_step_dev_-bf16", "adamw_step_scaled_", "sgd_step_", "adagrad_step_"]


@pytest.mark.parametrize("kernel", TRIPS)
def test_later_grid_stride_trips(ops, device, kernel):
    """the whole buffer compared after one launch whose grid-stride loop runs more than once; the one-launch steps publish
    their counter exactly once ([t + 1, 0]) with thousands of workgroups taking the ticket"""
    name, _, mir = kernel.partition("-")
    fused = name == "adamw_step_fused_"
    n = N_FUSED_TRIPS if fused else N_SCALAR_TRIPS
    (p, g, m, v), skip, hyper, t = _trip_case(device, n, 4 if fused else 1, tiny_p=(name == "adam_step_dev_"))
    if name == "adam_step_dev_":
        assert n > 4096 * 256
    skip_dev = skip.to(device)
    mirror = _mirror(n, MIRRORS.get(mir), device)
    what = f"{kernel} n={n}"
    if name in ("sgd_step_", "adagrad_step_"):
        if name == "sgd_step_":
            hy, state = dict(lr=0.05, mu=0.9, wd=0.09), m
            held = _hold(device, p, g, state)
            ops.sgd_step_(*(h.t for h in held), lr=0.05, momentum=0.9, weight_decay=0.09, skip=skip_dev)
            check = O.check_sgd
        else:
            hy, state = dict(lr=0.05, lr_decay=0.1, eps=1e-8, wd=0.09, step=7), v
            held = _hold(device, p, g, state)
            ops.adagrad_step_(*(h.t for h in held), lr=0.05, lr_decay=0.1, eps=1e-8, weight_decay=0.09, step=7, skip=skip_dev)
            check = O.check_adagrad
        got = _after(held, g, (p, state), skip, what=what)
        _report(what, check(got, (p, g, state), hy, skip=skip, what=what))
        return
    held = _hold(device, p, g, m, v)
    if name == "adamw_step_":
        hyper, skip = dict(hyper, bias="host"), None
        ops.adamw_step_(*(h.t for h in held), lr=hyper["lr"], step=t + 1, **_kw(hyper))
    elif name == "adamw_step_dev_":
        counter = torch.tensor([t], dtype=torch.int64, device=device)
        ops.adamw_step_dev_(*(h.t for h in held), counter, lr=hyper["lr"], skip=skip_dev, **_kw(hyper))
        assert counter.tolist() == [t + 1]
    elif name == "adamw_step_scaled_":
        sc = _Scaler(O.scaler_state(1.0, steps=t), device)
        _scaled_launch(ops, held, sc, skip_dev)
        assert sc.state() == dict(steps=t + 1, scale=1.0, found_inf=0, good_steps=1, loss_grad=0.25)
    else:
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        if fused:
            ops.adamw_step_fused_(*(h.t for h in held), counter, lr=hyper["lr"], skip=skip_dev,
                                  mirror=None if mirror is None else mirror.t, **_kw(hyper))
        else:
            lr_dev = torch.tensor([hyper["lr"]], dtype=torch.float32, device=device)
            ops.adam_step_dev_(*(h.t for h in held), counter, lr_dev, skip=skip_dev,
                               mirror=None if mirror is None else mirror.t, **_kw(hyper))
        assert counter.tolist() == [t + 1, 0], f"{what}: the counter is published once"
    got = _after(held, g, (p, m, v), skip, mirror, what=what)
    _report(what, O.check_adam(got, (p, g, m, v), hyper, skip=skip, what=what))


# ---------------------------------------------------------------- identical launches give identical bits
@pytest.mark.parametrize("kernel", ["adamw_step_", "adamw_step_dev_", "adamw_step_fused_", "adam_step_dev_",
                                    "adamw_step_scaled_", "sgd_step_", "adagrad_step_"])
def test_two_identical_launches_agree_bitwise(ops, device, kernel):
    n = 4099
    p, g, m, v = O.optim_inputs(n, _gen(n))
    b1, b2, t, _ = O.REGIMES["workload-9"]
    hyper = dict(HYP, b1=b1, b2=b2)
    skip = _skip_for(n).to(device)
    runs = []
    for _ in range(2):
        held = _hold(device, p, g, m, v)
        mirror = _mirror(n, torch.bfloat16, device)
        if kernel == "adamw_step_":
            ops.adamw_step_(*(h.t for h in held), lr=hyper["lr"], step=t + 1, **_kw(hyper))
        elif kernel == "adamw_step_dev_":
            ops.adamw_step_dev_(*(h.t for h in held), torch.tensor([t], device=device), lr=hyper["lr"], skip=skip, **_kw(hyper))
        elif kernel == "adamw_step_fused_":
            ops.adamw_step_fused_(*(h.t for h in held), torch.tensor([t, 0], device=device), lr=hyper["lr"], skip=skip,
                                  mirror=mirror.t, **_kw(hyper))
        elif kernel == "adam_step_dev_":
            ops.adam_step_dev_(*(h.t for h in held), torch.tensor([t, 0], device=device),
                               torch.tensor([hyper["lr"]], dtype=torch.float32, device=device), skip=skip, mirror=mirror.t,
                               **_kw(hyper))
        elif kernel == "adamw_step_scaled_":
            _scaled_launch(ops, held, _Scaler(O.scaler_state(1.0, steps=t), device), skip)
        elif kernel == "sgd_step_":
            ops.sgd_step_(held[0].t, held[1].t, held[2].t, lr=0.05, momentum=0.9, weight_decay=0.09, skip=skip)
        else:
            ops.adagrad_step_(held[0].t, held[1].t, held[3].t, lr=0.05, lr_decay=0.1, eps=1e-8, weight_decay=0.09, step=7,
                              skip=skip)
        runs.append([h.cpu() for h in held] + [mirror.cpu()])
    assert not _same_bits(runs[0][0], p)
    assert all(_same_bits(a, b) for a, b in zip(*runs)), kernel


# ---------------------------------------------------------------- the in-place clip, called directly
@pytest.mark.parametrize("norm", ["two", "inf"])
def test_grad_clip_direct(ops, device, norm):
    """ops.grad_clip_ on gradients of small integers: the total is exact, so what separates g * coef from its float64 value
    is four roundings of at most 2^-24 relative each (the root, its sum with 1e-6, the quotient, the product) and 1e-6f's own
    representation: 5 x 2^-24.  A threshold above the norm writes nothing."""
    norm_type = 2.0 if norm == "two" else math.inf
    gen = _gen(31)
    lengths = (1, 5, 8191, 8193, 3 * 8192 + 3)
    grads = [torch.randint(-2, 3, (n,), generator=gen).float() for n in lengths]
    grads[0][0] = 2.0
    for offset in (0, 1):                                     # the 16-byte path and the scalar one
        held = [Held(g, device, offset) for g in grads]
        table = ops.grad_table([h.t for h in held])
        total = sum(float((g.double() ** 2).sum()) for g in grads) if norm == "two" else 2.0
        want_norm = math.sqrt(total) if norm == "two" else total
        out = ops.grad_clip_(table, 1e30, norm_type)
        assert abs(float(out) - want_norm) <= 1e-6 * want_norm
        assert all(_same_bits(h.cpu(), g) for h, g in zip(held, grads)) and all(h.intact() for h in held)
        out = ops.grad_clip_(table, 0.5, norm_type)
        assert abs(float(out) - want_norm) <= 1e-6 * want_norm      # the norm before clipping
        coef = 0.5 / (want_norm + 1e-6)
        for h, g in zip(held, grads):
            assert h.intact()
            err = (h.cpu().double() - g.double() * coef).abs()
            assert bool((err <= 5 * 2.0 ** -24 * (g.double() * coef).abs()).all()), (norm, offset, g.numel())
