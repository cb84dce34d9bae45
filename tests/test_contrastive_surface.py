"""CPU-side checks of the embedding MLPs (src/models/contrastivemodel.py, src/models/basicmlp.py): the constructor,
attributes and state dict of the reference, the initialisation draws, the expert aggregation modes, the LR schedule, the
argument checks of the new C entry points, and a torch-CPU restatement that reproduces the reference fixture."""
import inspect
import math

import numpy as np
import pytest
import torch
from torch import nn

from tests import contrastive_ref as R
from tests.util import fill_state_from_numpy, golden

CT = dict(input_shape=40, hidden_layer=70, projection_size=37, output_shape=19, batch_size=6, num_samples=60,
          aggregation="concat", learning_rate=1e-3, weight_decay=0.09, epochs=500)
MLP = dict(input_shape=40, bottle_neck=1024, output_shape=305, batch_size=7, learning_rate=5e-6, aggregation="concat")


class _View:
    def __init__(self, v):
        self.v = v

    def get(self):
        return self.v


def _ct(**kw):
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    c = dict(CT)
    c.update(kw)
    return SpatioTemporalContrastiveModel(c)


def _mlp(**kw):
    from dvt_amd.models.basicmlp import BasicMLP
    c = dict(MLP)
    c.update(kw)
    return BasicMLP({k: _View(v) for k, v in c.items()})


def test_constructors_take_one_config():
    from dvt_amd.models.basicmlp import BasicMLP
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    assert list(inspect.signature(SpatioTemporalContrastiveModel.__init__).parameters)[1:] == ["config"]
    assert list(inspect.signature(BasicMLP.__init__).parameters)[1:] == ["config"]


def test_contrastive_attributes_and_state_dict_equal_the_fixture():
    m = _ct()
    for name in ("running_logits", "running_labels", "proj_list", "label_list", "train_iters_per_epoch", "loss",
                 "config", "encoder_net", "projector_net", "exclude_from_wt_decay", "compute_dtype"):
        assert hasattr(m, name), name
    assert m.train_iters_per_epoch == 10 and m.running_logits == [] and m.proj_list == []
    d = golden("contrastive_mlp.npz")
    assert list(m.state_dict()) == list(d["ct_keys"])
    for k, p in m.named_parameters():
        assert tuple(p.shape) == d[f"ct_grad:{k}"].shape, k
    assert isinstance(m.projector_net[3], nn.Dropout) and m.projector_net[3].p == 0.1


def test_basicmlp_attributes_and_state_dict_equal_the_fixture():
    m = _mlp()
    d = golden("contrastive_mlp.npz")
    assert list(m.state_dict()) == list(d["mlp_keys"])
    assert isinstance(m.loss, nn.CrossEntropyLoss) and isinstance(m.softmax, nn.LogSoftmax)
    assert m.fc4.out_features == 305 and m.batchnorm.num_features == 1024
    # plain dicts are accepted as well as confuse-style views
    from dvt_amd.models.basicmlp import BasicMLP
    assert list(BasicMLP(dict(MLP)).state_dict()) == list(d["mlp_keys"])


def test_same_seed_gives_the_reference_initial_weights():
    torch.manual_seed(3)
    m = _ct()
    torch.manual_seed(3)
    ref = [nn.Linear(40, 70, bias=False), nn.Linear(70, 70, bias=False), nn.Linear(70, 37), nn.Linear(37, 37),
           nn.Linear(37, 19)]
    ours = [m.encoder_net[0], m.encoder_net[3], m.encoder_net[5], m.projector_net[1], m.projector_net[4]]
    for a, b in zip(ours, ref):
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa, pb)
    torch.manual_seed(4)
    mm = _mlp()
    torch.manual_seed(4)
    fc1, fc2, fc3, fc4 = nn.Linear(40, 40), nn.Linear(40, 1024), nn.Linear(1024, 1024), nn.Linear(1024, 305)
    for a, b in ((mm.fc1, fc1), (mm.fc2, fc2), (mm.fc3, fc3), (mm.fc4, fc4)):
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)


def test_aggregation_modes():
    experts = [torch.randn(1, 24), torch.randn(1, 11), torch.randn(1, 5)]
    assert _ct(aggregation="none").expert_aggregation(experts) is experts[0]
    cat = _ct().expert_aggregation(experts)
    assert torch.equal(cat, torch.cat(experts, -1))
    for mode in ("mean_pool", "avg_pool", "collab_gate"):
        with pytest.raises(NotImplementedError, match=mode):
            _ct(aggregation=mode).expert_aggregation(experts)


def test_bottleneck_other_than_1024_fails_like_the_reference():
    m = _mlp(bottle_neck=512)
    with pytest.raises(RuntimeError, match="1024"):
        m(torch.randn(3, 40))


def test_optimizers():
    from dvt_amd import optim
    from dvt_amd.lr_scheduler import LinearWarmupCosineAnnealingLR
    (opt,), (sched,) = _ct().configure_optimizers()
    assert isinstance(opt, optim.Adam) and isinstance(sched, LinearWarmupCosineAnnealingLR)
    assert opt.param_groups[0]["weight_decay"] == 0.09 and sched.warmup_epochs == 50 and sched.max_epochs == 500
    assert sched.get_last_lr() == [0.0] and float(opt.lr_dev(0)) == 0.0        # epoch 0: warmup_start_lr
    o2 = _mlp().configure_optimizers()
    assert isinstance(o2, optim.Adam) and o2.param_groups[0]["weight_decay"] == 0.0


def _rule(e, w, M, base, s=0.0, eta=0.0, lr=None):
    """The chained rule of the issue, stated independently of the scheduler class."""
    if e == 0:
        return s
    if e < w:
        return lr + (base - s) / (w - 1)
    if e == w:
        return base
    if (e - 1 - M) % (2 * (M - w)) == 0:
        return lr + (base - eta) * (1 - math.cos(math.pi / (M - w))) / 2
    return (1 + math.cos(math.pi * (e - w) / (M - w))) / (1 + math.cos(math.pi * (e - w - 1) / (M - w))) * (lr - eta) + eta


def _closed(e, w, M, base, s=0.0, eta=0.0):
    if e < w:
        return s + e * (base - s) / max(1, w - 1)
    return eta + 0.5 * (base - eta) * (1 + math.cos(math.pi * (e - w) / (M - w)))


@pytest.mark.parametrize("epochs", [500, 5, 20])
def test_scheduler_follows_the_rule_in_both_forms(epochs):
    from dvt_amd.lr_scheduler import LinearWarmupCosineAnnealingLR
    base, w, M = 5e-6, epochs // 10, epochs
    p = nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=base)
    sched = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=w, max_epochs=M)
    lr, got, want = None, [], []
    for e in range(2 * M + 3):
        if e:
            opt.step()
            sched.step()
        lr = _rule(e, w, M, base, lr=lr)
        got.append(opt.param_groups[0]["lr"])
        want.append(lr)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-18)
    closed = [_closed(e, w, M, base) for e in range(2 * M + 3)]
    if w >= 1:      # the two forms agree at every epoch
        np.testing.assert_allclose(got, closed, rtol=1e-6, atol=1e-15)
        sched2 = LinearWarmupCosineAnnealingLR(torch.optim.SGD([p], lr=base), warmup_epochs=w, max_epochs=M)
        for e in (1, w, w + 3, M - 1, M + 1):
            with pytest.warns(UserWarning):
                sched2.step(e)
            assert sched2.get_last_lr()[0] == pytest.approx(closed[e], rel=1e-9, abs=1e-18)
    else:           # w = 0 (epochs < 10): the chained rule stays at warmup_start_lr through max_epochs
        assert all(v == 0.0 for v in got[:M + 1]) and all(v > 0 for v in closed[:M])
        assert got[M + 1] > 0      # ... until the periodic-restart branch at M + 1 adds a cosine step to it


def test_new_entry_points_validate_before_any_hip_call():
    import dvt_amd
    lib = dvt_amd._lib.load()
    p = 256
    checks = [
        ("dvt_bn1d_relu_fwd", lambda: lib.dvt_bn1d_relu_fwd(p, 8, p, 8, p, p, p, p, None, p, p, 1, 8, 1, 1e-5, 0.1, 1, 0, None)),
        ("dvt_bn1d_relu_fwd", lambda: lib.dvt_bn1d_relu_fwd(p, 8, p, 8, p, p, p, p, None, p, p, 4, 8, 3, 1e-5, 0.1, 1, 0, None)),
        ("dvt_bn1d_relu_fwd", lambda: lib.dvt_bn1d_relu_fwd(p, 4, p, 8, p, p, p, p, None, p, p, 4, 8, 1, 1e-5, 0.1, 1, 0, None)),
        ("dvt_bn1d_relu_fwd", lambda: lib.dvt_bn1d_relu_fwd(p, 8, p, 8, p, p, None, None, None, None, None, 4, 8, 1, 1e-5, 0.1, 0,
                                                    0, None)),
        ("dvt_bn1d_relu_bwd", lambda: lib.dvt_bn1d_relu_bwd(p, 8, p, 8, p, p, p, None, 8, p, p, 0, 4, 8, 1, 1, 0, None)),
        ("dvt_adam_step_dev", lambda: lib.dvt_adam_step_dev(p, p, p, p, 16, None, 0.9, 0.999, 1e-8, 0.0, p, None, None, 0, None)),
        ("dvt_adam_step_dev", lambda: lib.dvt_adam_step_dev(p, p, p, p, 16, p, 0.9, 0.999, 1e-8, 0.0, p, None, p, 0, None)),
        ("dvt_ce_labels_fwd", lambda: lib.dvt_ce_labels_fwd(p, 4, p, p, p, 3, 8, -100, 0, None)),
        ("dvt_ce_labels_bwd", lambda: lib.dvt_ce_labels_bwd(p, 8, None, p, p, p, 8, 3, 8, -100, 0, None)),
        ("dvt_gather_rows_ptr", lambda: lib.dvt_gather_rows_ptr(p, 4, 2, p, 8, 16, 0, None)),
    ]
    for name, call in checks:
        rc = call()
        assert rc == -1 and name.encode() in lib.dvt_last_error(), name
    rc = lib.dvt_bn1d_relu_fwd(p, 8, p, 8, p, p, p, p, None, p, p, 1, 8, 1, 1e-5, 0.1, 1, 0, None)
    assert rc == -1 and b"more than 1 value" in lib.dvt_last_error()


def _fixture_params(prefix, names_shapes, seed):
    mods = nn.Module()
    for k, shp in names_shapes:
        mods.register_parameter(k.replace(".", "__"), nn.Parameter(torch.empty(shp)))
    fill_state_from_numpy([(k, p) for (k, _), p in zip(names_shapes, mods.parameters())], seed)
    return {k: p.detach().double().requires_grad_(True) for (k, _), p in zip(names_shapes, mods.parameters())}


def test_cpu_restatement_reproduces_the_contrastive_fixture():
    d = golden("contrastive_mlp.npz")
    m = _ct()
    P = _fixture_params("ct", [(k, p.shape) for k, p in m.named_parameters()], int(d["ct_seed"]))
    xi, xj = torch.from_numpy(d["ct_x_i"]).double(), torch.from_numpy(d["ct_x_j"]).double()
    stats = [torch.zeros(70, dtype=torch.float64), torch.ones(70, dtype=torch.float64)]
    e, o = R.contrastive_forward(P, xi, [s.clone() for s in stats])
    np.testing.assert_allclose(e.detach().numpy(), d["ct_embedding"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o.detach().numpy(), d["ct_output"], rtol=1e-5, atol=1e-6)
    assert (d["ct_embedding"] >= 0).all()                  # the returned embedding is rectified
    loss = R.contrastive_step(P, xi, xj, stats)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(d["ct_loss"]), rel=1e-6)
    for k, p in P.items():
        np.testing.assert_allclose(p.grad.numpy(), d[f"ct_grad:{k}"], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(stats[0].numpy(), d["ct_bn:running_mean"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(stats[1].numpy(), d["ct_bn:running_var"], rtol=1e-5, atol=1e-7)
    assert int(d["ct_bn:num_batches_tracked"]) == 2


def test_cpu_restatement_reproduces_the_basicmlp_fixture():
    d = golden("contrastive_mlp.npz")
    m = _mlp()
    P = _fixture_params("mlp", [(k, p.shape) for k, p in m.named_parameters()], int(d["mlp_seed"]))
    x = torch.from_numpy(d["mlp_x"]).double()
    stats = [torch.zeros(1024, dtype=torch.float64), torch.ones(1024, dtype=torch.float64)]
    logits = R.mlp_forward(P, x, [s.clone() for s in stats])
    np.testing.assert_allclose(logits.detach().numpy(), d["mlp_logits"], rtol=1e-5, atol=1e-5)
    labels = torch.from_numpy(d["mlp_labels"])
    assert (labels == -100).sum() == 2
    loss = nn.CrossEntropyLoss()(R.mlp_forward(P, x, stats), labels)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(d["mlp_loss"]), rel=1e-6)
    for k, p in P.items():
        g = p.grad.numpy()
        if f"mlp_grad_norm:{k}" in d.files:
            assert np.linalg.norm(g) == pytest.approx(float(d[f"mlp_grad_norm:{k}"]), rel=1e-5)
            g = g[:32]
        np.testing.assert_allclose(g, d[f"mlp_grad:{k}"], rtol=1e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(stats[0].numpy(), d["mlp_bn:running_mean"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(stats[1].numpy(), d["mlp_bn:running_var"], rtol=1e-5, atol=1e-7)
