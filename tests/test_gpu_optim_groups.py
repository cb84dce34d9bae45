"""The grouped AdamW step and the weight EMA of csrc/optim_groups.hip on the GPU, with the recipe of
tests/test_gpu_optim.py: ``Held`` guard bands, ``optim_inputs``, two consecutive launches with the second from the state read
back, the regimes, and ``check_adam`` with its documented K -- applied to each group's elements with that group's rate and
decay (tests/optim_groups_ref.py).  Then the same launch through ``dp.FlatParameters`` on the small ViViT, eagerly and inside
a captured step.

Each case prints its worst error as a fraction of the budget (``[optim] ...``; run with -s to collect them)."""
import pytest
import torch

from tests import optim_groups_ref as G
from tests import optim_ref as O
from tests.test_gpu_optim import (HYP, MIRRORS, N_FUSED_TRIPS, Held, _after, _gen, _hold, _mirror, _report, _same_bits,
                                  _skip_for, _worse, ops)  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

NS = [4, 5, 63, 64, 65, 255, 257, 1027, 4099]
REGIME_IDS = ["workload-0", "small-1", "negligible-29999"]
LR = HYP["lr"]


def _lr(device, lr=LR):
    return torch.tensor([lr], dtype=torch.float32, device=device)


def _launch(ops, held, counter, lr_dev, table, b1, b2, skip=None, mirror=None, ema=None, decay=None):
    ops.adamw_groups_step_(*(h.t for h in held), counter, lr_dev, table, beta1=b1, beta2=b2, eps=HYP["eps"], skip=skip,
                           mirror=mirror, ema=ema, ema_decay=decay)


# ---------------------------------------------------------------- 1. per-group correctness
@pytest.mark.parametrize("regime", REGIME_IDS)
@pytest.mark.parametrize("mirror", list(MIRRORS))
def test_groups_step_per_group(ops, device, mirror, regime):
    """three groups over the 64-blocks as 0, 1, 2, 1, 0, ...; launch 1 on every block, launch 2 from the state read back
    with the skip mask; every group's elements under check_adam with lr = f32(f32(lr) f32(scale_g)), wd = wd_g"""
    b1, b2, t, K = O.REGIMES[regime]
    hyper = dict(lr=LR, eps=HYP["eps"], b1=b1, b2=b2)
    lr_dev = _lr(device)
    worst = None
    for n in NS:
        g64 = G.interleaved_groups(n)
        table = ops.adamw_group_table(g64, G.SCALES, G.DECAYS)
        p, g, m, v = O.optim_inputs(n, _gen(1000 + n), zero_state=(t == 0))
        held = _hold(device, p, g, m, v)
        mir = _mirror(n, MIRRORS[mirror], device)
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        for k, skip in enumerate((None, _skip_for(n))):
            _launch(ops, held, counter, lr_dev, table, b1, b2, None if skip is None else skip.to(device),
                    None if mir is None else mir.t)
            tag = f"adamw_groups_step_ {mirror} {regime} n={n} launch {k + 1}"
            assert counter.tolist() == [t + k + 1, 0], f"{tag}: the counter is published once, the ticket is back at 0"
            got = _after(held, g, (p, m, v), skip, mir, what=tag)
            worst = _worse(worst, G.check_groups(got, (p, g, m, v), g64, G.SCALES, G.DECAYS, dict(hyper, steps_taken=t + k),
                                                 K=K, skip=skip, what=tag))
            p, m, v = got
    _report(f"adamw_groups_step_ {mirror} {regime}", worst)


# ---------------------------------------------------------------- 2. the same arithmetic as the uniform step
@pytest.mark.parametrize("regime", REGIME_IDS)
def test_groups_step_is_bit_equal_to_the_uniform_step(ops, device, regime):
    """one group {1.0, wd}: bit-equal to adamw_step_fused_ on the same inputs; three groups: each group's elements
    bit-equal to adamw_step_fused_ run on them alone with lr = f32(lr scale_g)"""
    b1, b2, t, _ = O.REGIMES[regime]
    lr_dev = _lr(device)

    def uniform(p, g, m, v, lr, wd):
        held = _hold(device, p, g, m, v)
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        ops.adamw_step_fused_(*(h.t for h in held), counter, lr=lr, beta1=b1, beta2=b2, eps=HYP["eps"], weight_decay=wd)
        return [h.cpu() for h in (held[0], held[2], held[3])]

    for n in (5, 257, 4099):
        p, g, m, v = O.optim_inputs(n, _gen(2000 + n), zero_state=(t == 0))
        for ngroups in (1, 3):
            scales, decays = ((1.0,), (HYP["wd"],)) if ngroups == 1 else (G.SCALES, G.DECAYS)
            g64 = G.interleaved_groups(n, ngroups)
            held = _hold(device, p, g, m, v)
            counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
            _launch(ops, held, counter, lr_dev, ops.adamw_group_table(g64, scales, decays), b1, b2)
            got = _after(held, g, (p, m, v), None, what=f"bit-equal n={n}")
            for gi in range(ngroups):
                _, idx = G.group_elements(g64, gi, n)
                if idx.numel() == 0:
                    continue
                want = uniform(p[idx], g[idx], m[idx], v[idx], G.group_lr(LR, scales[gi]), decays[gi])
                for name, a, b in zip("pmv", got, want):
                    diff = (a[idx].view(torch.int32) != b.view(torch.int32)).nonzero()
                    assert diff.numel() == 0, (f"{regime} n={n} groups={ngroups} group {gi} {name}: first difference at "
                                               f"{int(idx[diff[0]])}: grouped {float(a[idx][diff[0]])!r}, uniform "
                                               f"{float(b[diff[0]])!r}")


# ---------------------------------------------------------------- 3. later trips of the grid-stride loop
def test_groups_step_later_grid_stride_trips(ops, device):
    n = N_FUSED_TRIPS
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first_trip = 256 * 8 * cus * 4
    assert n > first_trip, f"n = {n} does not exceed the grid of {cus} CUs ({first_trip} elements per trip)"
    block = (n - 200) >> 6
    assert block * 64 >= first_trip
    b1, b2, t, K = O.REGIMES["negligible-29999"]
    p, g, m, v = O.optim_inputs(n, _gen(n))
    skip = O.skip_mask(n, [block])
    g64 = G.interleaved_groups(n, 2)
    scales, decays = G.SCALES[:2], G.DECAYS[:2]
    held = _hold(device, p, g, m, v)
    mir = _mirror(n, torch.bfloat16, device)
    counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
    _launch(ops, held, counter, _lr(device), ops.adamw_group_table(g64, scales, decays), b1, b2, skip.to(device), mir.t)
    assert counter.tolist() == [t + 1, 0], "the counter is published once"
    got = _after(held, g, (p, m, v), skip, mir, what=f"grouped n={n}")
    _report(f"adamw_groups_step_ n={n}", G.check_groups(got, (p, g, m, v), g64, scales, decays,
                                                        dict(lr=LR, eps=HYP["eps"], b1=b1, b2=b2, steps_taken=t), K=K,
                                                        skip=skip, what=f"grouped n={n}"))


# ---------------------------------------------------------------- 4. the stand-alone EMA
@pytest.mark.parametrize("d", [0.5, 0.75])
def test_ema_update_exact(ops, device, d):
    """small integers: every product and the sum are exact in fp32, so the result equals the float64 one bit for bit"""
    decay = torch.tensor([d], dtype=torch.float32, device=device)
    for n in (1, 3, 64, 65, 4099, N_FUSED_TRIPS):
        gen = _gen(3000 + n)
        ema = torch.randint(-64, 65, (n,), generator=gen).float()
        p = torch.randint(-64, 65, (n,), generator=gen).float()
        he, hp = _hold(device, ema, p)
        ops.ema_update_(he.t, hp.t, decay)
        want = G.ema_step(ema.double(), p.double(), d=d)
        assert he.intact() and hp.intact() and _same_bits(hp.cpu(), p), f"n={n}: a guard band or p was written"
        assert torch.equal(he.cpu().double(), want) and _same_bits(he.cpu(), want.float()), f"n={n} d={d}"


def test_ema_update_random_and_a_new_decay(ops, device):
    decay = torch.tensor([0.9999], dtype=torch.float32, device=device)
    for n in (5, 257, 4099):
        gen = _gen(3100 + n)
        ema, p = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        ema[: n // 4] *= 1e-6                                      # an EMA far below the weights, and the reverse
        p[n // 4: n // 2] *= 1e-6
        he, hp = _hold(device, ema, p)
        decay.fill_(0.9999)
        ops.ema_update_(he.t, hp.t, decay)
        one = he.cpu()
        G.check_ema(one, ema, p, 0.9999, f"ema_update_ n={n}")
        assert he.intact() and hp.intact() and _same_bits(hp.cpu(), p)
        decay.fill_(0.25)                                          # the device scalar is followed without a rebuild
        ops.ema_update_(he.t, hp.t, decay)
        G.check_ema(he.cpu(), one, p, 0.25, f"ema_update_ n={n} d=0.25")
        assert not _same_bits(he.cpu(), one)


# ---------------------------------------------------------------- 5. the EMA fused into the grouped launch
@pytest.mark.parametrize("mirror", list(MIRRORS))
def test_fused_ema(ops, device, mirror):
    """the ema the grouped launch leaves == ema_update_ on the old ema and the p the same launch left, bit for bit, on
    skipped blocks too; ema=None leaves a neighbouring buffer alone.  The step with the EMA and the step without are held to
    the same float64 rule and leave the same moments; p is NOT compared bit for bit between them: the two kEma forms are two
    compilations of adam_update, and p * decay - step_size * q contracts the other way round on two lanes of a quad
    (measured, n = 65, element 23: -0.09721557050943375 with the EMA, -0.09721556305885315 without: one ulp)."""
    b1, b2, t, K = O.REGIMES["workload-9"]
    hyper = dict(lr=LR, eps=HYP["eps"], b1=b1, b2=b2, steps_taken=t)
    decay = torch.tensor([0.99], dtype=torch.float32, device=device)
    for n in (5, 65, 1027, 4099):
        g64 = G.interleaved_groups(n)
        table = ops.adamw_group_table(g64, G.SCALES, G.DECAYS)
        p, g, m, v = O.optim_inputs(n, _gen(4000 + n))
        ema = p + 0.01 * torch.randn(n, generator=_gen(n))
        skip = _skip_for(n)
        held = _hold(device, p, g, m, v)
        he = Held(ema, device)
        mir = _mirror(n, MIRRORS[mirror], device)
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        _launch(ops, held, counter, _lr(device), table, b1, b2, skip.to(device), None if mir is None else mir.t, he.t, decay)
        tag = f"fused ema {mirror} n={n}"
        assert counter.tolist() == [t + 1, 0], tag
        got = _after(held, g, (p, m, v), skip, mir, what=tag)
        G.check_groups(got, (p, g, m, v), g64, G.SCALES, G.DECAYS, hyper, K=K, skip=skip, what=tag)
        assert he.intact(), f"{tag}: a guard band of the ema was written"
        alone, hp = _hold(device, ema, got[0])
        ops.ema_update_(alone.t, hp.t, decay)
        assert _same_bits(he.cpu(), alone.cpu()), f"{tag}: the fused ema is not ema_update_ of the launch's own p"
        mask = skip.bool().repeat_interleave(64)[:n]
        assert not _same_bits(he.cpu()[mask], ema[mask]), f"{tag}: the ema of a skipped block did not move"
        # without ema: the same step, and the buffer next door is not touched
        held2 = _hold(device, p, g, m, v)
        idle = Held(ema, device)
        counter2 = torch.tensor([t, 0], dtype=torch.int64, device=device)
        _launch(ops, held2, counter2, _lr(device), table, b1, b2, skip.to(device))
        assert _same_bits(idle.cpu(), ema) and idle.intact()
        plain = _after(held2, g, (p, m, v), skip, what=f"{tag} without ema")
        G.check_groups(plain, (p, g, m, v), g64, G.SCALES, G.DECAYS, hyper, K=K, skip=skip, what=f"{tag} without ema")
        assert _same_bits(plain[1], got[1]) and _same_bits(plain[2], got[2]), f"{tag}: the EMA changed a moment"


# ---------------------------------------------------------------- 6. refusals
def test_refusals_write_nothing(ops, device):
    n = 257
    b1, b2, t, _ = O.REGIMES["negligible-29999"]
    p, g, m, v = O.optim_inputs(n, _gen(n))
    g64 = G.interleaved_groups(n)
    table = ops.adamw_group_table(g64, G.SCALES, G.DECAYS)
    decay = torch.tensor([0.99], dtype=torch.float32, device=device)
    lr_dev = _lr(device)

    def untouched(held, counter):
        torch.cuda.synchronize()
        assert counter.tolist() == [t, 0] and all(h.intact() for h in held)
        assert all(_same_bits(h.cpu(), x) for h, x in zip(held, (p, g, m, v, p)))

    for off in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
        held = [Held(x, device, o) for x, o in zip((p, g, m, v, p), off)]
        counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
        with pytest.raises(RuntimeError, match="dvt_adamw_groups_step: buffers must be 16-byte aligned"):
            _launch(ops, held[:4], counter, lr_dev, table, b1, b2, ema=held[4].t, decay=decay)
        untouched(held, counter)
    held = [Held(x, device) for x in (p, g, m, v, p)]
    counter = torch.tensor([t, 0], dtype=torch.int64, device=device)
    with pytest.raises(RuntimeError, match="dvt_adamw_groups_step: ema needs ema_decay_dev"):
        _launch(ops, held[:4], counter, lr_dev, table, b1, b2, ema=held[4].t)
    mir = _mirror(n, torch.bfloat16, device, 1)
    with pytest.raises(RuntimeError, match="dvt_adamw_groups_step: mirror must be bf16 / f16 and 8-byte aligned"):
        _launch(ops, held[:4], counter, lr_dev, table, b1, b2, mirror=mir.t)
    for k in (0, 256):                                               # the C entry's own check, behind the Python one
        forged = ops.AdamwGroupTable(table.group64, torch.zeros((256, 2), dtype=torch.float32, device=device))
        forged.ngroups = k
        with pytest.raises(RuntimeError, match="dvt_adamw_groups_step: ngroups must be in 1 .. 255"):
            _launch(ops, held[:4], counter, lr_dev, forged, b1, b2)
        with pytest.raises(ValueError, match="ngroups must be in 1 .. 255"):
            ops.adamw_group_table(g64, [1.0] * k, [0.0] * k)
    with pytest.raises(ValueError, match="map byte 2 at block 2 is not below ngroups = 2"):
        ops.adamw_group_table(g64.to(device), G.SCALES[:2], G.DECAYS[:2])
    untouched(held, counter)
    assert mir.intact() and bool(torch.isnan(mir.t.float()).all())
    he = Held(p, device, 1)
    with pytest.raises(RuntimeError, match="dvt_ema_update: buffers must be 16-byte aligned"):
        ops.ema_update_(he.t, held[0].t, decay)
    torch.cuda.synchronize()
    assert _same_bits(he.cpu(), p) and he.intact()


# ---------------------------------------------------------------- 7. FlatParameters end to end
def _vivit(compute_dtype):
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(1130)
    return ViViT(64, 16, 19, 4, dim=128, depth=2, heads=2, compute_dtype=compute_dtype).cuda()


def _write_grad(flat, g, leave_out):
    """the writers' protocol with a handed gradient: every sink but ``leave_out`` is written"""
    flat.zero_grad()
    flat.grad.copy_(g)
    for s in flat.sinks:
        if s.index != leave_out:
            s.mark_written()
    flat.finish_backward()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_flat_parameters_end_to_end(device, compute):
    from dvt_amd import optim
    from dvt_amd.dp import FlatParameters
    cdt = torch.float32 if compute == "fp32" else torch.bfloat16
    net = _vivit(cdt)
    flat = FlatParameters(net, compute_dtype=None if compute == "fp32" else cdt)
    lr, n = 1e-3, flat.total
    groups = optim.param_groups(net, lr, 0.05, layer_decay=0.75)
    with pytest.raises(RuntimeError, match="set_param_groups first"):
        flat.adamw_groups_step(lr)
    flat.set_param_groups(groups)
    scales, decays = zip(*flat.group_hyper)
    assert len(groups) == 12 and flat.group64.numel() * 64 == n
    real = torch.zeros(n, dtype=torch.bool)                         # elements that belong to a parameter
    for q, off in zip(flat.params, flat.offsets):
        real[off:off + q.numel()] = True
    assert int((~real).sum()) > 0
    _, g, _, _ = O.optim_inputs(n, _gen(7))
    g = torch.where(real, g, torch.zeros_like(g))
    left = len(flat.params) // 2                                    # the parameter nobody writes a gradient for
    p0 = flat.data.cpu()
    _write_grad(flat, g.to(device), left)
    g = flat.grad.cpu()                                             # (the slice nobody wrote holds zeros now)
    skip = flat.skip_mask.cpu()
    assert int(skip.sum()) == (flat.params[left].numel() + 63) // 64
    flat.adamw_groups_step(lr)
    torch.cuda.synchronize()
    assert flat.step_dev.tolist() == [1, 0] and flat.step_count == 1
    zeros = torch.zeros(n)
    got = (flat.data.cpu(), flat.exp_avg.cpu(), flat.exp_avg_sq.cpu())
    b1, b2, t, K = O.REGIMES["workload-0"]
    hyper = dict(lr=lr, eps=1e-8, b1=b1, b2=b2, steps_taken=0)
    _report(f"FlatParameters.adamw_groups_step {compute}",
            G.check_groups(got, (p0, g, zeros, zeros), flat.group64, scales, decays, hyper, K=K, skip=skip, what="flat"))
    assert all(not bool(x[~real].any()) for x in got), "alignment padding moved"
    lo = flat.offsets[left]
    hi = lo + flat.params[left].numel()
    assert _same_bits(got[0][lo:hi], p0[lo:hi]) and not bool(got[1][lo:hi].any()) and not bool(got[2][lo:hi].any())
    assert not _same_bits(got[0][real], p0[real])
    if flat.compute is not None:
        assert flat.compute_valid and _same_bits(flat.compute.cpu(), got[0].to(cdt))
        assert all(q._dvt_compute.data_ptr() == flat.compute.data_ptr() + 2 * off for q, off in zip(flat.params, flat.offsets))

    # the EMA: two more steps, the recursion on the weights read back
    ema = flat.enable_ema(0.99)
    assert _same_bits(ema.cpu(), got[0])
    weights = []
    for k in range(2):
        _write_grad(flat, (g * (1.0 + k)).to(device), left)
        flat.adamw_groups_step(lr)
        weights.append(flat.data.cpu())
    assert flat.step_dev.tolist() == [3, 0]

    def recursion(e, w1, w2):
        return G.ema_step(G.ema_step(e, w1, d=0.99), w2, d=0.99)
    from tests.rowwise_ref import assert_close, fp32_chain, ref64
    mag = torch.stack([t_.double().abs() for t_ in (got[0], *weights)]).amax(0)
    assert_close(flat.ema.cpu(), ref64(recursion, got[0], *weights), fp32_chain(recursion, got[0], *weights), mag, "flat.ema")

    # evaluation on the averaged weights
    x = torch.randn(2, 4, 3, 64, 64, generator=_gen(3)).to(device)
    net.eval()
    before, ema_before = flat.data.clone(), flat.ema.clone()
    with torch.no_grad():
        y_train = net(x).float().cpu()
        with flat.ema_weights():
            assert torch.equal(flat.data, ema_before) and torch.equal(flat.ema, before)
            q = flat.params[0]
            assert q.data_ptr() == flat.data.data_ptr() and torch.equal(q.detach().reshape(-1), ema_before[:q.numel()])
            assert flat.compute is None or not flat.compute_valid
            y_ema = net(x).float().cpu()
    assert _same_bits(flat.data.cpu(), before.cpu()) and _same_bits(flat.ema.cpu(), ema_before.cpu())
    assert bool(torch.isfinite(y_ema).all()) and not torch.equal(y_ema, y_train)

    # the state dict carries the EMA
    sd = flat.state_dict()
    assert _same_bits(sd["ema"], ema_before.cpu()) and float(sd["ema_decay_dev"]) == O.f32(0.99)
    other = FlatParameters(_vivit(cdt), compute_dtype=None)
    other.load_state_dict(sd)
    assert _same_bits(other.ema.cpu(), ema_before.cpu()) and other.step_dev.tolist() == [3, 0]
    flat.set_ema_decay(0.5)
    flat.ema_update()                                              # the stand-alone launch, on the same buffers
    G.check_ema(flat.ema.cpu(), ema_before.cpu(), before.cpu(), 0.5, "flat.ema_update")


# ---------------------------------------------------------------- 8. capture
def test_captured_step_follows_the_eager_one(device, monkeypatch):
    from dvt_amd import optim
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from tests.test_gpu_dp import _data, _model
    x, y = (t.to(device) for t in _data())

    def make():
        net = _model().cuda()
        flat = FlatParameters(net, compute_dtype=None)
        groups = optim.param_groups(net, 1e-3, 0.05, layer_decay=0.75)
        flat.set_param_groups(groups)
        flat.enable_ema(0.99)
        lr_dev = _lr(device, 1e-3)
        seed = torch.full((), flat.loss_scale, device=device)

        def step():
            flat.zero_grad()
            loss = net.loss(x, y)[0]
            loss.backward(seed)
            flat.finish_backward()
            flat.adamw_groups_step(lr_dev)
            return loss
        return flat, lr_dev, step, groups

    def run(flat, lr_dev, once):
        out = []
        for k in range(4):
            if k == 3:
                lr_dev.fill_(5e-4)                                  # a schedule writes the scalar between two steps
            once()
            out.append((flat.data.clone(), flat.ema.clone(), flat.step_dev.clone()))
        return out

    flat_e, lr_e, step_e, _ = make()
    start = flat_e.data.clone()
    eager = run(flat_e, lr_e, step_e)
    flat_g, lr_g, step_g, groups = make()
    assert torch.equal(flat_g.data, start)
    replay, _ = capture_step(step_g, warmup=1)
    torch.cuda.synchronize()
    flat_g.data.copy_(start)                                        # the warm-up and the capture moved the state: start again
    flat_g.ema.copy_(start)
    flat_g.exp_avg.zero_()
    flat_g.exp_avg_sq.zero_()
    flat_g.step_dev.zero_()
    graph = run(flat_g, lr_g, replay)
    torch.cuda.synchronize()
    for k, (e, r) in enumerate(zip(eager, graph)):
        assert e[2].tolist() == r[2].tolist() == [k + 1, 0], k
        assert torch.equal(e[0], r[0]) and torch.equal(e[1], r[1]), f"replay {k + 1} differs from the eager step"
    # the fourth step really ran at the new rate: an eager step at the old one lands elsewhere
    flat_o, lr_o, step_o, _ = make()
    for _ in range(4):
        step_o()
    assert not torch.equal(flat_o.data, eager[3][0])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)    # what the builders ask; no capture is opened
    with pytest.raises(RuntimeError, match="not inside a hipGraph capture"):
        flat_g.set_param_groups(groups)
    from dvt_amd import ops as _ops
    with pytest.raises(RuntimeError, match="not inside a hipGraph capture"):
        _ops.adamw_group_table(flat_g.group64, [1.0] * len(groups), [0.0] * len(groups))


# ---------------------------------------------------------------- 9. loss scaling
def test_loss_scaling_is_refused(device):
    from dvt_amd.dp import FlatParameters
    net = torch.nn.Linear(8, 4).cuda()
    flat = FlatParameters(net, compute_dtype=None)
    flat.set_param_groups([{"params": list(net.parameters()), "weight_decay": 0.01}])
    flat.enable_loss_scaling()
    before = flat.data.clone()
    with pytest.raises(NotImplementedError, match="adamw_step"):
        flat.adamw_groups_step(1e-3)
    assert torch.equal(flat.data, before) and flat.step_count == 0
