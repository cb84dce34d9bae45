"""LSTM baseline on the MI355X against CPU fp32 torch (nn.LSTM / nn.Linear / nn.BCELoss: the arithmetic the reference's
src/models/LSTM.py executes).  fp32 within 1e-4 relative L2; bf16 within 1e-2 against the same CPU fp32 computation on
bf16-rounded inputs and weights (the yardstick of test_gpu_ops.py)."""
import copy

import pytest
import torch
from torch import nn

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
BF16_TOL = 1e-2


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    dvt_amd._lib.load()
    return dvt_amd


def _tol(dtype):
    return F32_TOL if dtype == torch.float32 else BF16_TOL


def _round(t, dtype):
    return t.to(dtype).float()


def _layer_params(Fdim, H, gen):
    s = 1.0 / H ** 0.5
    return [((torch.rand(shape, generator=gen) * 2 - 1) * s) for shape in ((4 * H, Fdim), (4 * H, H), (4 * H,), (4 * H,))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Fdim,H", [(4, 16, 64, 32), (64, 200, 512, 512), (3, 7, 48, 64), (5, 1, 32, 16)])
def test_one_layer_fwd_bwd_matches_torch(dvt, dtype, B, T, Fdim, H):
    gen = torch.Generator().manual_seed(B * 1000 + T * 10 + H)
    w_ih, w_hh, b_ih, b_hh = _layer_params(Fdim, H, gen)
    x = torch.randn(B, T, Fdim, generator=gen)
    gout = torch.randn(B, T, H, generator=gen)
    glast = torch.randn(B, H, generator=gen)
    if dtype != torch.float32:                       # the oracle sees the operands the kernels see
        x, w_ih, w_hh = _round(x, dtype), _round(w_ih, dtype), _round(w_hh, dtype)

    ref = nn.LSTM(Fdim, H, 1, batch_first=True)
    with torch.no_grad():
        for p, v in zip((ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v)
    xr = x.clone().requires_grad_(True)
    out_r, _ = ref(xr)
    ((out_r * gout).sum() + (out_r[:, -1] * glast).sum()).backward()

    ps = [v.cuda().requires_grad_(True) for v in (w_ih, w_hh, b_ih, b_hh)]
    xg = x.cuda().to(dtype).requires_grad_(True)
    out, last = dvt.functional.lstm_layer(xg, *ps)
    torch.autograd.backward([out, last], [gout.cuda().to(dtype), glast.cuda().to(dtype)])
    torch.cuda.synchronize()

    tol = _tol(dtype)
    assert rel_l2(out.float(), out_r) < tol
    assert rel_l2(last.float(), out_r[:, -1]) < tol
    assert rel_l2(xg.grad.float(), xr.grad) < tol
    for p, r, name in zip(ps, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0),
                          ("dW_ih", "dW_hh", "db_ih", "db_hh")):
        assert p.grad.dtype == torch.float32
        e = rel_l2(p.grad, r.grad)
        assert e < tol, f"{name} rel {e:.2e}"


def _reference_model(n_features, hidden, layers, dropout):
    ref = nn.Module()
    ref.lstm = nn.LSTM(input_size=n_features, hidden_size=hidden, batch_first=True, num_layers=layers, dropout=dropout)
    ref.linear = nn.Linear(hidden, 15)
    return ref


def _ref_loss(ref, x, y):
    out, _ = ref.lstm(x)
    return nn.BCELoss()(torch.sigmoid(ref.linear(out[:, -1])), y)


def _ours(dvt, ref, n_features, hidden, layers, dropout, dtype):
    from dvt_amd.models.LSTM import LSTMRegressor
    m = LSTMRegressor(n_features=n_features, hidden_size=hidden, seq_len=0, batch_size=0, num_layers=layers,
                      dropout=dropout, learning_rate=5e-5, criterion=nn.BCELoss())
    m.load_state_dict(ref.state_dict())
    m.compute_dtype = dtype
    return m.cuda()


def _batch(x, y):
    return {"experts": [x[i:i + 1].cuda() for i in range(x.shape[0])],
            "label": [y[i:i + 1].cuda() for i in range(y.shape[0])]}


def _round_weights(ref, dtype):
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.startswith("lstm.weight") or n == "linear.weight":
                p.copy_(_round(p, dtype))


@pytest.fixture(scope="module")
def reference_shape_case():
    """The reference configuration (src/main.py:40-42) with dropout 0, one batch, and its CPU fp32 loss + gradients for
    fp32 weights and for bf16-rounded weights / inputs."""
    torch.manual_seed(1234)
    ref = _reference_model(4608, 512, 4, 0.0)
    x = torch.randn(64, 200, 4608)
    y = (torch.rand(64, 15) < 0.3).float()
    cases = {}
    for dtype in (torch.float32, torch.bfloat16):
        r = copy.deepcopy(ref)
        xx = x
        if dtype != torch.float32:
            _round_weights(r, dtype)
            xx = _round(x, dtype)
        loss = _ref_loss(r, xx, y)
        loss.backward()
        cases[dtype] = (r, float(loss), {n: p.grad.clone() for n, p in r.named_parameters()})
    return x, y, cases


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_training_step_at_the_reference_shape(dvt, reference_shape_case, dtype):
    x, y, cases = reference_shape_case
    ref, ref_loss, ref_grads = cases[dtype]
    m = _ours(dvt, ref, 4608, 512, 4, 0.0, dtype)
    loss = m.training_step(_batch(x, y), 0)
    loss.backward()
    torch.cuda.synchronize()
    tol = _tol(dtype)
    assert abs(float(loss) - ref_loss) <= tol * abs(ref_loss)
    for n, p in m.named_parameters():
        e = rel_l2(p.grad, ref_grads[n])
        assert e < tol, f"{n} rel {e:.2e}"


def test_bce_clamp_with_saturated_logits(dvt):
    torch.manual_seed(5)
    ref = _reference_model(64, 32, 2, 0.0)
    with torch.no_grad():                 # logits of +-300 for most classes: sigmoid is 0 or 1 in fp32, log clamps at -100
        ref.linear.bias.copy_(torch.tensor([300.0, -300.0] * 7 + [0.5]))
    x = torch.randn(4, 16, 64)
    y = (torch.rand(4, 15) < 0.5).float()
    loss_r = _ref_loss(ref, x, y)
    loss_r.backward()
    m = _ours(dvt, ref, 64, 32, 2, 0.0, torch.float32)
    logits = m(x.cuda())
    assert float(logits.abs().max()) > 100
    loss = m.training_step(_batch(x, y), 0)
    loss.backward()
    assert float(loss_r) > 20                                     # the clamp is what bounds it
    assert abs(float(loss) - float(loss_r)) <= 1e-4 * float(loss_r)
    for n, p in m.named_parameters():
        g = ref.get_parameter(n).grad
        assert rel_l2(p.grad, g) < F32_TOL, n


def test_dropout_between_layers_only(dvt):
    torch.manual_seed(9)
    x = torch.randn(4, 16, 64).cuda()
    ref2 = _reference_model(64, 32, 2, 0.0)
    m0 = _ours(dvt, ref2, 64, 32, 2, 0.0, torch.float32)
    m2 = _ours(dvt, ref2, 64, 32, 2, 0.2, torch.float32)
    with torch.no_grad():
        y0 = m0(x)
        m2.train()
        y_train = m2(x)
        m2.eval()
        y_eval = m2(x)
    assert torch.equal(y_eval, y0)                 # eval mode: deterministic, equal to dropout 0
    assert not torch.equal(y_train, y0)            # train mode: masks between the two layers
    ref1 = _reference_model(64, 32, 1, 0.0)        # one layer: nn.LSTM applies no dropout at all
    a = _ours(dvt, ref1, 64, 32, 1, 0.2, torch.float32).train()
    b = _ours(dvt, ref1, 64, 32, 1, 0.0, torch.float32)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


def test_three_adam_steps_match_torch(dvt):
    torch.manual_seed(11)
    ref = _reference_model(64, 32, 2, 0.0)
    m = _ours(dvt, ref, 64, 32, 2, 0.0, torch.float32)
    init = {n: p.detach().clone() for n, p in ref.named_parameters()}
    opt_r = torch.optim.Adam(ref.parameters(), lr=5e-5)
    opt = m.configure_optimizers()
    for step in range(3):
        x = torch.randn(4, 16, 64)
        y = (torch.rand(4, 15) < 0.3).float()
        opt_r.zero_grad()
        _ref_loss(ref, x, y).backward()
        opt_r.step()
        opt.zero_grad()
        m.training_step(_batch(x, y), step).backward()
        opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        r = ref.get_parameter(n).detach()
        assert rel_l2(p.detach().cpu() - init[n], r - init[n]) < 1e-3, n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_training_step_is_bitwise_reproducible(dvt, dtype):
    torch.manual_seed(3)
    ref = _reference_model(256, 128, 2, 0.0)
    m = _ours(dvt, ref, 256, 128, 2, 0.0, dtype)
    x = torch.randn(16, 50, 256)
    y = (torch.rand(16, 15) < 0.3).float()
    runs = []
    for _ in range(2):
        m.zero_grad()
        loss = m.training_step(_batch(x, y), 0)
        loss.backward()
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_validation_step_collects_sigmoid_outputs(dvt):
    torch.manual_seed(4)
    ref = _reference_model(64, 32, 2, 0.0)
    m = _ours(dvt, ref, 64, 32, 2, 0.0, torch.float32).eval()
    x = torch.randn(4, 16, 64)
    y = (torch.rand(4, 15) < 0.3).float()
    with torch.no_grad():
        loss = m.validation_step(_batch(x, y), 0)
        out_r, _ = ref.lstm(x)
        p_r = torch.sigmoid(ref.linear(out_r[:, -1]))
    assert len(m.running_logits) == 1 and len(m.running_labels) == 1
    assert rel_l2(m.running_logits[0], p_r) < F32_TOL
    assert torch.equal(m.running_labels[0].cpu(), y)
    assert abs(float(loss) - float(nn.BCELoss()(p_r, y))) < 1e-4
    assert "val_loss" in m.logged if hasattr(m, "logged") else True
