"""CPU-side checks of LARS: the constructor's refusals, defaults and state names, the optimizer choice of
SpatioTemporalContrastiveModel.configure_optimizers, the LR-scalar wiring, the argument checks of the three C entry points,
the chunk plan's arithmetic, and the float64 restatement (tests/lars_ref.py) against three hand-worked cases."""
import ctypes as C
import inspect

import pytest
import torch
from torch import nn

from tests import lars_ref

CT = dict(input_shape=40, hidden_layer=70, projection_size=37, output_shape=19, batch_size=6, num_samples=60,
          aggregation="concat", learning_rate=1e-3, weight_decay=0.09, epochs=500)


def _ct(**kw):
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    c = dict(CT)
    c.update(kw)
    return SpatioTemporalContrastiveModel(c)


def test_constructor_refusals_are_the_reference_ones():
    from dvt_amd.optim import LARS
    p = [nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-0.1), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4),
               dict(lr=0.1, nesterov=True), dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            LARS(p, **kw)
    LARS(p, lr=0.0)                                               # zero is not negative
    LARS(p, lr=0.1, nesterov=True, momentum=0.9)
    with pytest.raises(TypeError):
        LARS(p)                                                   # lr is required


def test_defaults_and_state_names():
    from dvt_amd import optim
    sig = inspect.signature(optim.LARS.__init__).parameters
    assert list(sig)[1:] == ["params", "lr", "momentum", "dampening", "weight_decay", "nesterov", "trust_coefficient", "eps"]
    assert [sig[k].default for k in list(sig)[3:]] == [0, 0, 0, False, 0.001, 1e-8]
    opt = optim.LARS([nn.Parameter(torch.zeros(3))], lr=0.1)
    g = opt.param_groups[0]
    assert {k: g[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "trust_coefficient", "eps")} == dict(
        lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False, trust_coefficient=0.001, eps=1e-8)
    assert isinstance(opt, torch.optim.Optimizer) and opt.state_dict()["state"] == {}
    # a state dict written by torch's SGD (the names pl_bolts' LARS uses too) loads
    p = nn.Parameter(torch.ones(3))
    sgd = torch.optim.SGD([p], lr=0.1, momentum=0.9)
    p.grad = torch.ones(3)
    sgd.step()
    sd = sgd.state_dict()
    assert list(sd["state"][0]) == ["momentum_buffer"]
    lars = optim.LARS([p], lr=0.1, momentum=0.9)
    lars.load_state_dict({"state": sd["state"], "param_groups": lars.state_dict()["param_groups"]})
    assert torch.equal(lars.state[p]["momentum_buffer"], torch.ones(3))


def test_configure_optimizers_adam_without_the_key_lars_with_it():
    from dvt_amd import optim
    from dvt_amd.lr_scheduler import LinearWarmupCosineAnnealingLR
    (opt,), _ = _ct().configure_optimizers()
    assert isinstance(opt, optim.Adam)
    (opt,), _ = _ct(optimizer="adam").configure_optimizers()
    assert isinstance(opt, optim.Adam)
    with pytest.raises(ValueError, match="sgd"):
        _ct(optimizer="sgd").configure_optimizers()
    m = _ct(optimizer="lars", momentum=0.9)
    (opt,), (sched,) = m.configure_optimizers()
    assert isinstance(opt, optim.LARS) and isinstance(sched, LinearWarmupCosineAnnealingLR)
    assert sched.warmup_epochs == 50 and sched.max_epochs == 500
    decayed, excluded = opt.param_groups
    assert decayed["weight_decay"] == 0.09 and excluded["weight_decay"] == 0.0
    for g in (decayed, excluded):
        assert g["momentum"] == 0.9 and g["trust_coefficient"] == 0.0001 and g["dampening"] == 0 and not g["nesterov"]
    names = {id(p): k for k, p in m.named_parameters()}
    # The reference's substring rule ('bias', 'bn') catches the four biases.  No parameter name contains 'bn': the
    # BatchNorm1d is encoder_net.2, so its bias is excluded through 'bias' and its weight is decayed with the matrices.
    assert [names[id(p)] for p in excluded["params"]] == ["encoder_net.2.bias", "encoder_net.5.bias", "projector_net.1.bias",
                                                          "projector_net.4.bias"]
    assert [names[id(p)] for p in decayed["params"]] == ["encoder_net.0.weight", "encoder_net.2.weight", "encoder_net.3.weight",
                                                         "encoder_net.5.weight", "projector_net.1.weight",
                                                         "projector_net.4.weight"]
    assert len(names) == 10
    assert float(opt.lr_dev(0)) == 0.0 and float(opt.lr_dev(1)) == 0.0         # epoch 0: warmup_start_lr, both groups


def test_scheduler_writes_every_groups_lr_scalar():
    from dvt_amd import optim
    from dvt_amd.lr_scheduler import LinearWarmupCosineAnnealingLR
    a, b = nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(2))
    opt = optim.LARS([{"params": [a]}, {"params": [b], "weight_decay": 0.0, "lr": 0.5}], lr=0.25, weight_decay=0.1)
    assert float(opt.lr_dev(0)) == 0.25 and float(opt.lr_dev(1)) == 0.5 and opt.lr_dev(0).dtype == torch.float32
    sched = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=3, max_epochs=10)
    assert [float(opt.lr_dev(i)) for i in (0, 1)] == [0.0, 0.0]
    with pytest.warns(UserWarning):            # torch: scheduler stepped before the optimizer; nothing to step here
        sched.step()
    assert [float(opt.lr_dev(i)) for i in (0, 1)] == [0.125, 0.25]
    opt.param_groups[0]["lr"] = 2.0
    opt.sync_lr()
    assert [float(opt.lr_dev(i)) for i in (0, 1)] == [2.0, 0.25]
    assert opt.step() is None                  # no gradients: no launch, no GPU needed


def test_entry_points_validate_before_any_hip_call():
    import dvt_amd
    from dvt_amd import _lib
    lib = dvt_amd._lib.load()
    for name in ("dvt_lars_plan", "dvt_lars_sumsq", "dvt_lars_step"):
        assert name in _lib.SIGNATURES
    Seg, Info = _lib.STRUCTS["dvt_lars_seg"], _lib.STRUCTS["dvt_lars_plan_info"]
    assert C.sizeof(Seg) == 56 and [f for f, _ in Seg._fields_][:4] == ["param", "grad", "buf", "mirror"]
    t, p = C.cast(256, C.POINTER(Seg)), 256
    info, one, zero = Info(), (C.c_int64 * 1)(5), (C.c_int64 * 1)(0)
    bf16, f32 = _lib.BF16, _lib.F32
    checks = [
        ("dvt_lars_plan", lambda: lib.dvt_lars_plan(None, 1, C.byref(info), None)),
        ("dvt_lars_plan", lambda: lib.dvt_lars_plan(C.cast(one, C.c_void_p), 1, None, None)),
        ("dvt_lars_plan", lambda: lib.dvt_lars_plan(C.cast(zero, C.c_void_p), 1, C.byref(info), None)),
        ("dvt_lars_sumsq", lambda: lib.dvt_lars_sumsq(None, 1, 1, p, p, None)),
        ("dvt_lars_sumsq", lambda: lib.dvt_lars_sumsq(t, 1, 1, None, p, None)),
        ("dvt_lars_sumsq", lambda: lib.dvt_lars_sumsq(t, 1, 1, p, None, None)),
        ("dvt_lars_sumsq", lambda: lib.dvt_lars_sumsq(t, 2, 1, p, p, None)),              # fewer chunks than segments
        ("dvt_lars_step", lambda: lib.dvt_lars_step(None, 1, 1, p, p, 0.9, 0.0, 0, 1e-3, 1e-8, p, 0, 0, None)),
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, None, p, 0.9, 0.0, 0, 1e-3, 1e-8, p, 0, 0, None)),
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, None, 0.9, 0.0, 0, 1e-3, 1e-8, p, 0, 0, None)),
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, p, 0.9, 0.0, 0, 1e-3, 1e-8, None, 0, 0, None)),
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, p, 0.9, 0.0, 0, 1e-3, 1e-8, p, 1, f32, None)),   # fp32 mirror
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, p, 0.9, 0.0, 0, 1e-3, 1e-8, p, 1, 7, None)),
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, p, 0.0, 0.0, 1, 1e-3, 1e-8, p, 1, bf16, None)),  # nesterov, no momentum
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, 1, 1, p, p, 0.9, 0.5, 1, 1e-3, 1e-8, p, 0, 0, None)),     # nesterov, dampening
        ("dvt_lars_step", lambda: lib.dvt_lars_step(t, -1, 1, p, p, 0.9, 0.0, 0, 1e-3, 1e-8, p, 0, 0, None)),
    ]
    for name, call in checks:
        rc = call()
        assert rc == -1 and name.encode() in lib.dvt_last_error(), name
    # n == 0 is a no-op whatever the pointers are
    assert lib.dvt_lars_sumsq(None, 0, 0, None, None, None) == 0
    assert lib.dvt_lars_step(None, 0, 0, None, None, 0.9, 0.0, 0, 1e-3, 1e-8, None, 0, 0, None) == 0
    assert lib.dvt_lars_plan(None, 0, C.byref(info), None) == 0 and info.blocks == 0 and info.workspace_bytes == 0


def test_plan_arithmetic():
    from dvt_amd import ops
    chunk = ops.lars_plan([1]).chunk
    assert chunk >= 64 and chunk % 4 == 0
    numels = [1, 3, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 4608 * 2048, 305]
    plan = ops.lars_plan(numels)
    per = [-(-n // chunk) for n in numels]
    assert per[5:9] == [1, 1, 2, 3]
    assert plan.chunk == chunk and plan.blocks == sum(per)
    assert plan.chunk_begin == tuple(sum(per[:i]) for i in range(len(numels) + 1))
    assert plan.workspace_bytes == 2 * 4 * plan.blocks                  # two fp32 partial sums per chunk
    assert plan.grid_cap == 0 or plan.grid_cap >= 1
    # a segment's chunking depends on its numel alone
    assert ops.lars_plan([7, 2 * chunk + 5]).chunk_begin[2] - ops.lars_plan([7, 2 * chunk + 5]).chunk_begin[1] == 3
    with pytest.raises(RuntimeError, match="dvt_lars_plan"):
        ops.lars_plan([4, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lars_table([(torch.zeros(4), torch.zeros(4), None, None, 0.0)])


def _one(p, g, buf=None, **kw):
    (q,), (b,) = lars_ref.lars_step([torch.tensor(p)], [torch.tensor(g)], [None if buf is None else torch.tensor(buf)], **kw)
    return q.tolist(), None if b is None else b.tolist()


def test_reference_on_three_hand_worked_cases():
    # quirk 1: weight_decay == 0 -> no trust scaling at all, plain SGD whatever trust_coefficient is
    assert _one([1.0, 2.0], [0.5, -1.0], lr=0.5, trust_coefficient=123.0) == ([0.75, 2.5], None)
    # quirk 2: a zero norm drops the decay term too.  p = 0: a raw gradient step; g = 0: nothing moves
    assert _one([0.0, 0.0], [3.0, 4.0], lr=0.25, weight_decay=0.5, eps=0.0) == ([-0.75, -1.0], None)
    assert _one([3.0, 4.0], [0.0, 0.0], lr=0.25, weight_decay=0.5, eps=0.0) == ([3.0, 4.0], None)
    # the scaled step itself: |p| = |g| = 5, q = 1 * 5 / (5 + 1 * 5) = 1/2, d = (g + p) / 2 = [3.5, 3.5]
    kw = dict(lr=1.0, weight_decay=1.0, trust_coefficient=1.0, eps=0.0, momentum=0.5, dampening=0.5)
    # quirk 3: on the first step buf is d itself, not (1 - dampening) d
    assert _one([3.0, 4.0], [4.0, 3.0], **kw) == ([-0.5, 0.5], [3.5, 3.5])
    # ... afterwards buf = 0.5 * [2, 2] + 0.5 * [3.5, 3.5] = [2.75, 2.75]
    assert _one([3.0, 4.0], [4.0, 3.0], [2.0, 2.0], **kw) == ([0.25, 1.25], [2.75, 2.75])
    # nesterov: d + momentum buf, buf = 0.5 * [2, 2] + [3.5, 3.5] = [4.5, 4.5], step [5.75, 5.75]
    kw.update(dampening=0.0, nesterov=True)
    assert _one([3.0, 4.0], [4.0, 3.0], [2.0, 2.0], **kw) == ([-2.75, -1.75], [4.5, 4.5])
    # the fp32 chain and the chunked order are the same code
    for extra in (dict(dtype=torch.float32), dict(order="chunks", chunk=1)):
        assert _one([3.0, 4.0], [4.0, 3.0], [2.0, 2.0], **kw, **extra) == ([-2.75, -1.75], [4.5, 4.5])
    # a parameter without a gradient is skipped
    (q,), (b,) = lars_ref.lars_step([torch.tensor([1.0, 2.0])], [None], [None], lr=1.0, momentum=0.9, weight_decay=0.1)
    assert q.tolist() == [1.0, 2.0] and b is None
