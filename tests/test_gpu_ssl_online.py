"""GPU checks of the online probe (csrc/probe.hip, models/evaluator.py, metrics.SSLOnlineEval) on the MI355X: the threshold
sweep against the scikit-learn fixture, the three-launch probe step against the float64 restatement
(tests/ssl_online_ref.py), gradient accumulation, the dropout masks, reproducibility, eval mode, and the callback on a
SpatioTemporalContrastiveModel."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import ssl_online_ref as R
from tests.util import golden, rel_l2

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2, torch.float16: 1e-2}          # tests/test_gpu_contrastive.py's table
SHAPES = [(256, 305, 512, 15), (7, 40, 32, 19), (1024, 2048, 512, 15)]
LR = 0.005


def _probe(D, H, C, dtype, p, seed):
    from dvt_amd.models.evaluator import SSLEvaluator
    torch.manual_seed(seed)
    e = SSLEvaluator(D, C, n_hidden=H, p=p)
    with torch.no_grad():
        bn = e.block_forward[3]
        bn.weight.copy_(1 + 0.1 * torch.randn(H))
        bn.bias.copy_(0.1 * torch.randn(H))
        bn.running_mean.copy_(0.1 * torch.randn(H))
        bn.running_var.copy_(0.5 + torch.rand(H))
    e.compute_dtype = dtype
    return e.cuda().train()


def _batch(B, D, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g).to(dtype)                    # rounded inputs: the CPU sees the same values
    y = (torch.rand(B, C, generator=g) < 0.2).float()
    return x, y


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["256x305x512x15", "7x40x32x19", "1024x2048x512x15"])
def test_first_probe_step_against_the_float64_restatement(shape, dtype):
    B, D, H, C = shape
    e = _probe(D, H, C, dtype, 0.0, seed=B + D)
    x, y = _batch(B, D, C, dtype, seed=H + C)
    P, stats = R.params64(e), R.stats64(e)
    before = {k: v.detach().clone() for k, v in e.named_parameters()}
    loss_r, prob_r, h_r, grads_r = R.step(P, x.double(), y.double(), stats)
    saved = {}
    loss, prob = e.step(x.cuda(), y.cuda(), LR, saved=saved)
    torch.cuda.synchronize()
    tol = TOL[dtype]
    ours = {k: rel_l2(p.grad, grads_r[k]) for k, p in e.named_parameters()}
    fwd = dict(loss=abs(float(loss) - float(loss_r)) / abs(float(loss_r)), prob=rel_l2(prob, prob_r), h=rel_l2(saved["h"], h_r))
    print(f"{shape} {dtype}: forward {fwd} gradients {ours}")
    assert loss.dim() == 0 and loss.is_cuda and prob.dtype == torch.float32 and saved["h"].dtype == dtype
    assert all(v <= tol for v in fwd.values()), fwd
    bn = e.block_forward[3]
    assert rel_l2(bn.running_mean, stats[0]) <= tol and rel_l2(bn.running_var, stats[1]) <= tol
    assert int(bn.num_batches_tracked) == 1
    if dtype == torch.float32:
        assert all(v <= tol for v in ours.values()), ours
    else:
        # the project's parity rule: at most twice the deviation of torch's own eager modules in this dtype from the same
        # float64 restatement, on the same inputs and the same GPU
        t = copy.deepcopy(_probe(D, H, C, dtype, 0.0, seed=B + D)).to(dtype)
        out = t.block_forward(x.cuda())
        nn.BCELoss()(torch.sigmoid(out.float()), y.cuda()).backward()
        theirs = {k: rel_l2(p.grad, grads_r[k]) for k, p in t.named_parameters()}
        print(f"{shape} {dtype}: torch eager gradients {theirs}")
        for k in ours:
            assert ours[k] <= 2 * theirs[k], (k, ours[k], theirs[k])
    for k, p in e.named_parameters():                                # torch.optim.SGD on the fp32 masters, exactly
        assert torch.equal(p.detach(), before[k] - LR * p.grad), k


@pytest.mark.parametrize("zero_grad", [False, True])
def test_two_steps_accumulate_unless_zeroed(zero_grad):
    B, D, H, C = 64, 40, 32, 19
    e = _probe(D, H, C, torch.float32, 0.0, seed=3)
    P, stats = R.params64(e), R.stats64(e)
    batches = [_batch(B, D, C, torch.float32, seed=s) for s in (11, 12)]
    acc = None
    for x, y in batches:
        _, _, _, g = R.step(P, x.double(), y.double(), stats)
        acc = g if acc is None or zero_grad else {k: acc[k] + g[k] for k in g}
        with torch.no_grad():
            for k in R.KEYS:
                P[k] -= LR * acc[k]
        e.step(x.cuda(), y.cuda(), LR, accumulate=not zero_grad)
    for k, p in e.named_parameters():
        assert rel_l2(p.grad, acc[k]) <= 1e-4, k
        assert rel_l2(p, P[k]) <= 1e-6, k
    assert int(e.block_forward[3].num_batches_tracked) == 2


def test_dropout_masks_scale_and_backward_reuse():
    """p = 0.1: with W1 = I (H = D) and a BatchNorm that is the identity on batch-normalised columns, h shows both masks;
    the gradient of W1 shows that the backward used the forward's masks."""
    from dvt_amd import functional as F
    B, D, C = 256, 64, 15
    e = _probe(D, D, C, torch.float32, 0.1, seed=5)
    with torch.no_grad():
        e.block_forward[2].weight.copy_(torch.eye(D))
        e.block_forward[3].weight.fill_(1.0)
        e.block_forward[3].bias.fill_(4.0)                         # every pre-dropout activation positive
    x, y = _batch(B, D, C, torch.float32, seed=6)
    F.manual_seed(77)
    saved = {}
    e.step(x.cuda(), y.cuda(), 0.0, accumulate=False, rng_offset=0, saved=saved)
    z, h = saved["z"], saved["h"]
    xg = x.cuda()
    keep1 = z != 0                                                   # z = drop(x) I: the first mask, directly
    assert 0.07 < float((~keep1).float().mean()) < 0.13
    assert rel_l2(z[keep1], xg[keep1] / 0.9) <= 1e-6
    mean, inv = saved["stats"][0], saved["stats"][1]
    pre = (z - mean) * inv + 4.0
    assert float(pre.min()) > 0
    keep2 = h != 0
    assert 0.07 < float((~keep2).float().mean()) < 0.13
    assert rel_l2(h[keep2], pre[keep2] / 0.9) <= 1e-5
    assert float((keep1 ^ keep2).float().mean()) > 0.1               # two different masks
    # the restatement with exactly these masks reproduces every gradient
    e2 = _probe(D, D, C, torch.float32, 0.1, seed=5)
    with torch.no_grad():
        e2.block_forward[2].weight.copy_(torch.eye(D))
        e2.block_forward[3].weight.fill_(1.0)
        e2.block_forward[3].bias.fill_(4.0)
    P, stats = R.params64(e2), R.stats64(e2)
    _, prob_r, _, g = R.step(P, x.double(), y.double(), stats, mask1=keep1.cpu().double(), mask2=keep2.cpu().double(), p=0.1)
    for k, p in e.named_parameters():
        assert rel_l2(p.grad, g[k]) <= 1e-4, k


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16", "fp16"])
def test_step_is_bitwise_reproducible(dtype):
    from dvt_amd import functional as F
    B, D, H, C = 256, 305, 512, 15
    x, y = _batch(B, D, C, dtype, seed=8)
    outs = []
    for _ in range(2):
        F.manual_seed(5)
        e = _probe(D, H, C, dtype, 0.1, seed=7)
        loss, prob = e.step(x.cuda(), y.cuda(), LR, rng_offset=12)
        outs.append((loss.clone(), prob.clone(), [p.detach().clone() for p in e.parameters()],
                     e.block_forward[3].running_var.clone()))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize("dtype", DT, ids=["fp32", "bf16", "fp16"])
def test_eval_mode_uses_the_running_statistics_and_moves_nothing(dtype):
    B, D, H, C = 33, 305, 512, 15
    e = _probe(D, H, C, dtype, 0.1, seed=9).eval()
    x, y = _batch(B, D, C, dtype, seed=10)
    P, stats = R.params64(e), R.stats64(e)
    state = copy.deepcopy(e.state_dict())
    with torch.no_grad():
        _, logits_r = R.forward(P, x.double(), stats, False)
        prob_r = torch.sigmoid(logits_r)
        loss_r = R.bce(prob_r, y.double())
    loss, prob = e.evaluate(x.cuda(), y.cuda())
    logits = e(x.cuda())
    again = e.evaluate(x.cuda(), y.cuda())[1]
    assert rel_l2(prob, prob_r) <= TOL[dtype] and rel_l2(logits, logits_r) <= TOL[dtype]
    assert abs(float(loss) - float(loss_r)) <= TOL[dtype] * abs(float(loss_r))
    assert torch.equal(prob, again)                                  # no dropout drawn
    for k, v in e.state_dict().items():
        assert torch.equal(v, state[k]), k
    one = e.evaluate(x[:1].cuda(), y[:1].cuda())[1]                  # a single row is fine in eval mode
    assert rel_l2(one, prob_r[:1]) <= TOL[dtype]
    with pytest.raises(NotImplementedError, match="1024"):
        e.train().step(x[:1].cuda(), y[:1].cuda(), LR)


def test_sweep_counts_equal_the_fixture_and_sklearn():
    from dvt_amd import metrics, ops
    g = golden("ssl_online.npz")
    probs, labels = torch.from_numpy(g["probs"]).cuda(), torch.from_numpy(g["labels"]).cuda()
    counts, support = ops.multilabel_sweep_counts(probs, labels, g["thresholds"])
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (6, 3, 15)
    assert np.array_equal(counts.cpu().numpy(), g["counts"]) and np.array_equal(support.cpu().numpy(), g["support"])

    class M:
        running_logits, running_labels, logged = [probs[:50], probs[50:]], [labels[:50], labels[50:]], {}

        def log(self, k, v, **kw):
            self.logged[k] = v

    m = M()
    scalars, rows = metrics.SSLOnlineEval(z_dim=40, num_classes=15).on_shared_end(m, "val")
    assert list(scalars) == list(g["keys"]) and len(rows) == 20
    assert np.abs(np.array([scalars[k] for k in g["keys"]]) - g["scalars"]).max() < 1e-12
    assert m.running_logits == [] and m.running_labels == []


def _contrastive(dtype):
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    from tests.test_contrastive_surface import CT
    torch.manual_seed(21)
    m = SpatioTemporalContrastiveModel(dict(CT))
    m.compute_dtype = dtype
    return m.cuda().train()


def _loader_batch(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    cuts = (0, 24, 35, 40)
    x = torch.randn(B, 40, generator=g)
    experts = [[r[None, a:b].cuda() for a, b in zip(cuts, cuts[1:])] for r in x]
    labels = [(torch.rand(C, generator=g) < 0.3).float() for _ in range(B)]
    return {"x_i_experts": experts, "x_j_experts": experts, "label": labels}, x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_callback_on_the_contrastive_model(dtype):
    from dvt_amd import metrics
    m = _contrastive(dtype)
    cb = metrics.SSLOnlineEval(drop_p=0.1, z_dim=37, num_classes=15)
    cb.on_pretrain_routine_start(None, m)
    probe = m.non_linear_evaluator
    assert probe.compute_dtype == dtype and next(probe.parameters()).is_cuda
    own = [(k, p) for k, p in m.named_parameters() if not k.startswith("non_linear_evaluator")]
    for _, p in own:
        p.grad = torch.randn_like(p)
    before = {k: (p.detach().clone(), p.grad.clone()) for k, p in own}
    w_before = probe.block_forward[2].weight.detach().clone()
    batch, _ = _loader_batch(12, 15, seed=1)
    loss = cb.on_train_batch_end(None, m, None, batch, 0, 0)
    assert loss.dim() == 0 and loss.is_cuda and m.logged["train/online/loss"] is loss
    for k, p in own:
        assert torch.equal(p.detach(), before[k][0]) and torch.equal(p.grad, before[k][1]), k
    assert int(m.encoder_net[2].num_batches_tracked) == 1            # the callback's own forward, in training mode
    assert not torch.equal(probe.block_forward[2].weight.detach(), w_before)
    assert int(probe.block_forward[3].num_batches_tracked) == 1

    m.eval()
    sizes, xs, ys = (12, 9, 5), [], []
    for i, n in enumerate(sizes):
        vb, _ = _loader_batch(n, 15, seed=30 + i)
        cb.on_validation_batch_end(None, m, None, vb, i, 0)
        ys.append(torch.stack(vb["label"]))
    assert "val/online/loss" in m.logged and len(m.running_logits) == 3
    assert all(t.is_cuda and t.dtype == torch.float32 for t in m.running_logits)
    probs = torch.cat(m.running_logits).cpu().numpy()
    want = R.sklearn_scalars(probs, torch.cat(ys).numpy(), metrics.ONLINE_THRESHOLDS)
    scalars, rows = cb.on_validation_epoch_end(None, m)
    assert len(scalars) == 24 and list(scalars) == list(want) and set(scalars) <= set(m.logged)
    assert max(abs(scalars[k] - want[k]) for k in want) < 1e-12
    assert m.running_logits == [] and m.running_labels == [] and len(rows) == 20
    assert int(m.encoder_net[2].num_batches_tracked) == 1 and int(probe.block_forward[3].num_batches_tracked) == 1
