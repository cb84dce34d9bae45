"""GPU checks of the embedding MLPs (csrc/embed_mlp.hip and the models above it) on the MI355X: BatchNorm1d-after-ReLU
against float64 torch, Adam against torch.optim.Adam, the label cross-entropy against nn.CrossEntropyLoss, both models
against the reference fixture, step_views against two forward calls, the projector dropout, and a captured step."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import contrastive_ref as R
from tests.util import fill_state_from_numpy, golden, rel_l2

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2, torch.float16: 1e-2}


def _bn_case(B, C, S, dtype, training, seed):
    from dvt_amd import functional as F
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(S * B, C, generator=g) * 2 + 0.5).to(dtype)           # rounded inputs: the CPU sees the same values
    dy = torch.randn(S * B, C, generator=g).to(dtype)
    bn = nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(C, generator=g))
        bn.bias.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.3 * torch.rand(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    ref = nn.BatchNorm1d(C).double()
    ref.load_state_dict(bn.state_dict())
    bn.cuda().train(training)
    ref.train(training)
    zr = z.double().requires_grad_(True)
    outs = [ref(torch.relu(zr[s * B:(s + 1) * B])) for s in range(S)]       # S successive torch calls
    yr = torch.cat(outs)
    yr.backward(dy.double())
    zg = z.cuda().requires_grad_(True)
    y = F.batch_norm1d_relu(zg, bn, segments=S)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return y, zg.grad, bn, yr, zr.grad, ref


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("training", [True, False])
def test_bn1d_relu_against_float64_torch(dtype, training):
    tol = TOL[dtype]
    for C in (305, 1024, 2048):
        for B in (2, 3, 64, 256):
            for S in (1, 2):
                y, dz, bn, yr, dzr, ref = _bn_case(B, C, S, dtype, training, seed=C * 1000 + B * 10 + S)
                what = f"C={C} B={B} S={S}"
                assert y.dtype == dtype
                assert rel_l2(y, yr) <= tol, what
                assert rel_l2(dz, dzr) <= tol * (4 if training and B <= 3 else 1), what
                assert rel_l2(bn.weight.grad, ref.weight.grad) <= tol, what
                assert rel_l2(bn.bias.grad, ref.bias.grad) <= tol, what
                assert rel_l2(bn.running_mean, ref.running_mean) <= 1e-5, what
                assert rel_l2(bn.running_var, ref.running_var) <= 1e-5, what
                assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == (S if training else 0), what


def test_bn1d_relu_is_bitwise_reproducible():
    for dtype in DT:
        a = _bn_case(256, 2048, 2, dtype, True, seed=5)
        b = _bn_case(256, 2048, 2, dtype, True, seed=5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[2].weight.grad, b[2].weight.grad) and torch.equal(a[2].running_var, b[2].running_var)


def test_bn1d_relu_wide_mean_small_spread():
    """Post-ReLU columns whose mean is 1e5 spreads above zero: the centred variance keeps the normalised output to the
    fp32 rounding of the mean (E[x^2] - mean^2 in fp32 would lose the variance entirely: its error is ~1e3 times it)."""
    from dvt_amd import functional as F
    B, C = 256, 305
    z = 1000.0 + 0.01 * torch.randn(B, C, dtype=torch.float64)
    bn = nn.BatchNorm1d(C).cuda()
    y = F.batch_norm1d_relu(z.float().cuda(), bn)
    ref = nn.BatchNorm1d(C).double()(z.float().double())
    assert rel_l2(y, ref) <= 2e-2


def test_adam_matches_torch_with_coupled_decay_and_moving_lr():
    from dvt_amd import optim
    torch.manual_seed(0)
    shapes = [(70, 40), (70,), (305, 37)]
    ps = [torch.randn(s) for s in shapes]
    ours = [nn.Parameter(p.clone().cuda()) for p in ps]
    ref = [nn.Parameter(p.clone().double()) for p in ps]
    o = optim.Adam(ours, lr=1e-3, weight_decay=0.09)
    t = torch.optim.Adam(ref, lr=1e-3, weight_decay=0.09)
    lrs = [0.0, 1e-3, 3e-3, 2e-4, 5e-3]
    for step, lr in enumerate(lrs):
        grads = [torch.randn(s) for s in shapes]
        for p, q, g in zip(ours, ref, grads):
            p.grad, q.grad = g.cuda(), g.double()
        for grp in (o.param_groups[0], t.param_groups[0]):
            grp["lr"] = lr
        o.step()
        t.step()
        torch.cuda.synchronize()
        for p, q in zip(ours, ref):
            assert rel_l2(p, q) <= 1e-6, step                  # fp32 state against float64 torch
            assert rel_l2(o.state[p]["exp_avg"], t.state[q]["exp_avg"]) <= 5e-5
            assert rel_l2(o.state[p]["exp_avg_sq"], t.state[q]["exp_avg_sq"]) <= 5e-5
        if step == 0:                    # lr = 0 at epoch 0: parameters unchanged, moments moved
            for p, q in zip(ours, ps):
                assert torch.equal(p.detach().cpu(), q)
            assert float(o.state[ours[0]]["exp_avg"].abs().sum()) > 0
    assert int(o.state[ours[0]]["step"][0]) == len(lrs)


def test_flat_adam_step_and_its_16bit_mirror():
    from dvt_amd import dp, ops, optim
    torch.manual_seed(1)
    net = nn.Sequential(nn.Linear(40, 70), nn.Linear(70, 19)).cuda()
    ref = [p.detach().double().cpu().clone().requires_grad_(True) for p in net.parameters()]
    flat = dp.FlatParameters(net, compute_dtype=torch.bfloat16)
    opt = optim.Adam(net.parameters(), lr=2e-3, weight_decay=0.09)
    t = torch.optim.Adam(ref, lr=2e-3, weight_decay=0.09)
    for step in range(5):
        flat.zero_grad()
        for p, q in zip(net.parameters(), ref):
            g = torch.randn(p.shape)
            p.grad.copy_(g.cuda())
            p._dvt_sink.mark_written()
            q.grad = g.double()
        flat.finish_backward()
        flat.adam_step(opt.lr_dev(0), weight_decay=0.09)
        t.step()
    torch.cuda.synchronize()
    for p, q in zip(net.parameters(), ref):
        assert rel_l2(p, q) <= 1e-6
        assert torch.equal(p._dvt_compute.cpu(), p.detach().cpu().to(torch.bfloat16))


def test_cross_entropy_against_torch():
    from dvt_amd import functional as F
    torch.manual_seed(2)
    for dtype in (torch.float32, torch.bfloat16):
        x = (3 * torch.randn(64, 305)).to(dtype)
        y = torch.randint(0, 305, (64,))
        y[::7] = -100
        xr = x.double().requires_grad_(True)
        lr_ = nn.CrossEntropyLoss()(xr, y)
        lr_.backward()
        xg = x.cuda().requires_grad_(True)
        loss = F.cross_entropy(xg, y.cuda())
        loss.backward()
        assert abs(float(loss.detach()) - float(lr_.detach())) <= 1e-5 * max(1.0, abs(float(lr_.detach())))
        assert rel_l2(xg.grad, xr.grad) <= TOL[dtype]
        assert float(xg.grad[::7].abs().sum()) == 0.0
    bad = torch.tensor([0, 305, 2], device="cuda")            # out of range: NaN, not an out-of-bounds read
    assert torch.isnan(F.cross_entropy(torch.randn(3, 305, device="cuda"), bad))


def test_gather_rows_ptr_concat_and_cast():
    from dvt_amd import ops
    torch.manual_seed(3)
    rows = [[torch.randn(24, device="cuda"), torch.randn(11, device="cuda", dtype=torch.bfloat16),
             torch.randn(5, device="cuda")] for _ in range(9)]
    for dtype in DT:
        got = ops.gather_rows_ptr(rows, 40, dtype, "cuda")
        want = torch.stack([torch.cat([t.float() for t in r]) for r in rows]).to(dtype)
        assert torch.equal(got, want)


def _models(dtype):
    from dvt_amd.models.basicmlp import BasicMLP
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    from tests.test_contrastive_surface import CT, MLP
    d = golden("contrastive_mlp.npz")
    ct = SpatioTemporalContrastiveModel(dict(CT))
    fill_state_from_numpy(ct.named_parameters(), int(d["ct_seed"]))
    ct.projector_net[3].p = 0.0
    mlp = BasicMLP(dict(MLP))
    fill_state_from_numpy(mlp.named_parameters(), int(d["mlp_seed"]))
    for m in (ct, mlp):
        m.compute_dtype = dtype
        m.cuda().train()
    return d, ct, mlp


def _experts(x):
    cuts = (0, 24, 35, 40)
    return [[torch.from_numpy(r[None, a:b]).cuda() for a, b in zip(cuts, cuts[1:])] for r in x]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_contrastive_model_reproduces_the_fixture(dtype):
    d, ct, _ = _models(dtype)
    # bf16: the BatchNorm backward at B = 6 subtracts two projections of dy, which magnifies the 16-bit rounding of the
    # activations in the gradients below it; fp32 pins the arithmetic at 1e-4
    tol, gtol = (1e-4, 1e-4) if dtype == torch.float32 else (2e-2, 0.25)
    emb, out = ct(torch.from_numpy(d["ct_x_i"]).cuda())
    assert rel_l2(emb, torch.from_numpy(d["ct_embedding"])) <= tol
    assert rel_l2(out, torch.from_numpy(d["ct_output"])) <= tol
    ct.encoder_net[2].reset_running_stats()
    batch = {"x_i_experts": _experts(d["ct_x_i"]), "x_j_experts": _experts(d["ct_x_j"]), "label": list(range(6))}
    loss = ct.training_step(batch, 0)
    loss.backward()
    assert abs(float(loss) - float(d["ct_loss"])) <= tol * 10 * abs(float(d["ct_loss"]))
    for k, p in ct.named_parameters():
        assert rel_l2(p.grad, torch.from_numpy(d[f"ct_grad:{k}"])) <= gtol, k
    bn = ct.encoder_net[2]
    assert rel_l2(bn.running_mean, torch.from_numpy(d["ct_bn:running_mean"])) <= tol
    assert rel_l2(bn.running_var, torch.from_numpy(d["ct_bn:running_var"])) <= tol
    assert int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_basicmlp_reproduces_the_fixture(dtype):
    d, _, mlp = _models(dtype)
    tol, gtol = (1e-4, 1e-4) if dtype == torch.float32 else (2e-2, 0.25)      # (B = 7: see the contrastive test)
    logits = mlp(torch.from_numpy(d["mlp_x"]).cuda())
    assert rel_l2(logits, torch.from_numpy(d["mlp_logits"])) <= tol
    mlp.batchnorm.reset_running_stats()
    batch = {"x_i_experts": [torch.from_numpy(r[None]).cuda() for r in d["mlp_x"]], "label": list(d["mlp_labels"])}
    loss = mlp.training_step(batch, 0)
    loss.backward()
    assert abs(float(loss) - float(d["mlp_loss"])) <= tol * 10 * abs(float(d["mlp_loss"]))
    for k, p in mlp.named_parameters():
        g = p.grad
        if f"mlp_grad_norm:{k}" in d.files:
            assert abs(float(g.double().norm()) / float(d[f"mlp_grad_norm:{k}"]) - 1) <= gtol, k
            g = g[:32]
        assert rel_l2(g, torch.from_numpy(d[f"mlp_grad:{k}"])) <= gtol, k
    assert rel_l2(mlp.batchnorm.running_var, torch.from_numpy(d["mlp_bn:running_var"])) <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_views_equals_two_forward_calls(dtype):
    _, ct, _ = _models(dtype)
    import copy
    twin = copy.deepcopy(ct)
    torch.manual_seed(4)
    xi, xj = torch.randn(6, 40, device="cuda"), torch.randn(6, 40, device="cuda")
    (ei, oi), (ej, oj) = ct.step_views(xi, xj)
    ei2, oi2 = twin(xi)
    ej2, oj2 = twin(xj)
    for a, b in ((ei, ei2), (oi, oi2), (ej, ej2), (oj, oj2)):
        assert rel_l2(a, b) <= (1e-6 if dtype == torch.float32 else 1e-2)
    b1, b2 = ct.encoder_net[2], twin.encoder_net[2]
    assert rel_l2(b1.running_mean, b2.running_mean) <= 1e-6 and rel_l2(b1.running_var, b2.running_var) <= 1e-6
    assert int(b1.num_batches_tracked) == int(b2.num_batches_tracked) == 2


def test_projector_dropout_mask_recovery():
    """Dropout(0.1) after the projector's second ReLU: with the last Linear set to the identity the output shows the
    mask directly -- zeros where dropped, relu(h) / 0.9 elsewhere."""
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    from tests.test_contrastive_surface import CT
    c = dict(CT)
    c["output_shape"] = c["projection_size"]
    m = SpatioTemporalContrastiveModel(c).cuda().train()
    m.compute_dtype = torch.float32
    with torch.no_grad():
        m.projector_net[4].weight.copy_(torch.eye(37))
        m.projector_net[4].bias.zero_()
        m.projector_net[1].bias.fill_(5.0)             # every pre-dropout activation positive
    x = torch.randn(256, 40, device="cuda")
    e, out = m(x)
    m.eval()
    _, keep_all = m(x)
    m.train()
    pre = torch.relu(e @ m.projector_net[1].weight.T + m.projector_net[1].bias)
    dropped = out == 0
    frac = float(dropped.float().mean())
    assert 0.07 < frac < 0.13
    assert rel_l2(out[~dropped], pre[~dropped] / 0.9) <= 1e-5


def test_captured_step_across_a_scheduler_step_equals_eager():
    from dvt_amd import dp, graph
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    from tests.test_contrastive_surface import CT

    def make():
        torch.manual_seed(9)
        c = dict(CT)
        c["epochs"] = 20                                # warmup 2 epochs: the LR changes at every epoch
        m = SpatioTemporalContrastiveModel(c).cuda().train()
        m.projector_net[3].p = 0.0
        flat = dp.FlatParameters(m, compute_dtype=torch.bfloat16)
        (opt,), (sched,) = m.configure_optimizers()
        opt.param_groups[0]["initial_lr"] = 1e-3
        return m, flat, opt, sched

    torch.manual_seed(10)
    xi, xj = torch.randn(6, 40, device="cuda"), torch.randn(6, 40, device="cuda")
    x = torch.cat([xi, xj]).to(torch.bfloat16)

    def stepper(m, flat, opt):
        from dvt_amd import functional as F

        def step():
            flat.zero_grad()
            _, out = m._run(x, 2)
            loss = m._loss_rows(F.l2_normalize(out))
            loss.backward()
            flat.finish_backward()
            flat.adam_step(opt.lr_dev(0), weight_decay=0.09)
            return loss
        return step

    plan = [2, 3, 2]                                    # steps per epoch, scheduler.step() between epochs
    m1, f1, o1, s1 = make()
    step = stepper(m1, f1, o1)
    for i, n in enumerate(plan):
        for _ in range(n):
            step()
        s1.step()
    m2, f2, o2, s2 = make()
    replay, _ = graph.capture_step(stepper(m2, f2, o2), warmup=1)
    # capture_step ran warm-up + capture steps: start again from the same state
    torch.cuda.synchronize()
    m3, f3, o3, s3 = make()
    f2.data.copy_(f3.data)
    f2.exp_avg.zero_()
    f2.exp_avg_sq.zero_()
    f2.step_dev.zero_()
    f2.sync_compute_copy()
    for b2, b3 in zip(m2.buffers(), m3.buffers()):
        b2.copy_(b3)
    for i, n in enumerate(plan):
        for _ in range(n):
            replay()
        s2.step()
    torch.cuda.synchronize()
    assert torch.equal(f1.data, f2.data)
    assert torch.equal(m1.encoder_net[2].running_var, m2.encoder_net[2].running_var)
