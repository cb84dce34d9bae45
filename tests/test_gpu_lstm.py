"""LSTM baseline on the MI355X against CPU fp32 torch (nn.LSTM / nn.Linear / nn.BCELoss: the arithmetic the reference's
src/models/LSTM.py executes).  fp32 within 1e-4 relative L2; bf16 within 1e-2 against the same CPU fp32 computation on
bf16-rounded inputs and weights (the yardstick of test_gpu_ops.py); fp16 within four times the error of the CPU fp32
restatement that rounds G, h_t, dG and dx to fp16 where the kernels do (tests/rowwise_ref.py lstm_layer_restated).

The chain's two entry points are also called directly (float64 recurrence, NaN-poisoned buffers), and the forward step's
K loop gets a two-step run whose second step sums tau * (+-1) per 8-wide group: tests/test_rowwise_cpu.py proves that
operand set sees a dropped, doubled or moved group, chunk or wave share."""
import copy
import math

import pytest
import torch
from torch import nn

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
BF16_TOL = 1e-2
# fp16: 4 x the restatement's own relative L2 error against CPU fp32 torch, measured on the CPU over every (B, T, F, H) of
# test_one_layer_fwd_bwd_matches_torch: outputs 1.92e-4 .. 2.76e-4, gradients 2.27e-4 .. 4.05e-4
FP16_TOL_OUT = 4 * 2.76e-4
FP16_TOL_GRAD = 4 * 4.05e-4
KSTEP_TOL = 1e-4    # tests/test_rowwise_cpu.py: a fault moves some gate by >= 0.64, the reference's fp32 evaluation by <= 3.5e-8


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    dvt_amd._lib.load()
    return dvt_amd


def _tol(dtype, grad=False):
    if dtype == torch.float16:
        return FP16_TOL_GRAD if grad else FP16_TOL_OUT
    return F32_TOL if dtype == torch.float32 else BF16_TOL


def _round(t, dtype):
    return t.to(dtype).float()


def _layer_params(Fdim, H, gen):
    s = 1.0 / H ** 0.5
    return [((torch.rand(shape, generator=gen) * 2 - 1) * s) for shape in ((4 * H, Fdim), (4 * H, H), (4 * H,), (4 * H,))]


# (17, 3, 32, 48): a ragged second batch tile, wave 1 gets half a chunk; (16, 5, 8, 160): wave 0 takes a second pass
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,T,Fdim,H", [(4, 16, 64, 32), (64, 200, 512, 512), (3, 7, 48, 64), (5, 1, 32, 16),
                                        (17, 3, 32, 48), (33, 2, 16, 80), (16, 5, 8, 160), (1, 4, 16, 16)])
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

    tol, gtol = _tol(dtype), _tol(dtype, grad=True)
    assert rel_l2(out.float(), out_r) < tol
    assert rel_l2(last.float(), out_r[:, -1]) < tol
    assert rel_l2(xg.grad.float(), xr.grad) < gtol
    for p, r, name in zip(ps, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0),
                          ("dW_ih", "dW_hh", "db_ih", "db_hh")):
        assert p.grad.dtype == torch.float32
        e = rel_l2(p.grad, r.grad)
        assert e < gtol, f"{name} rel {e:.2e}"


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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
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


# ---------------------------------------------------------------- the chain's entry points, called directly
def _poison(*ts):
    for t in ts:
        if t is not None:
            t.fill_(math.nan)


def _seq_fwd_poisoned(dvt, G, w_hh, b_ih, b_hh, B, T, want_last):
    """ops.lstm_seq_fwd with every output NaN before the launch (torch.empty inside ops hands out NaN-filled memory)"""
    from tests.test_gpu_rowwise import guarded
    with guarded(dvt.ops):
        return dvt.ops.lstm_seq_fwd(G, w_hh, b_ih, b_hh, B, T, want_last=want_last)


@pytest.mark.parametrize("variant", ["no_bias", "dh_seq", "dh_last", "both"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_lstm_seq_fwd_bwd_direct(dvt, dtype, variant):
    from tests import rowwise_ref as R
    from tests.test_gpu_rowwise import guarded
    B, T, H = 17, 3, 48
    gen = torch.Generator().manual_seed(77)
    G = (torch.randn(B * T, 4 * H, generator=gen, dtype=torch.float64)).to(dtype)
    w_hh = ((torch.rand(4 * H, H, generator=gen, dtype=torch.float64) * 2 - 1) / H ** 0.5).to(dtype)
    b_ih = b_hh = None
    if variant != "no_bias":
        b_ih, b_hh = (torch.randn(4 * H, generator=gen) * 0.1 for _ in range(2))
    dh_seq = torch.randn(B, T, H, generator=gen, dtype=torch.float64).to(dtype) if variant in ("no_bias", "dh_seq", "both") else None
    dh_last = torch.randn(B, H, generator=gen, dtype=torch.float64).to(dtype) if variant in ("dh_last", "both") else None
    dev = lambda t: None if t is None else t.cuda()

    h_out, h_prev, gates, c, h_last = _seq_fwd_poisoned(dvt, dev(G), dev(w_hh), dev(b_ih), dev(b_hh), B, T, True)
    torch.cuda.synchronize()
    assert not torch.isnan(gates).any() and not torch.isnan(c).any() and not torch.isnan(h_out.float()).any()
    assert not torch.isnan(h_prev.float()).any() and not torch.isnan(h_last.float()).any()
    assert torch.equal(h_prev[:, 0], torch.zeros_like(h_prev[:, 0]))
    assert torch.equal(h_prev[:, 1:], h_out[:, :-1])
    assert torch.equal(h_last, h_out[:, -1])
    # every step against the float64 step from the state the kernel itself carried into it (h_prev, c of the step before):
    # a 16-bit h_t that lands on the other side of a rounding boundary than float64's does not leak into the next check
    G3, hp, ck = G.reshape(B, T, 4 * H), h_prev.cpu(), c.cpu()
    gmag = float(G.double().abs().max())
    for t in range(T):
        cprev = ck[:, t - 1] if t > 0 else torch.zeros(B, H)
        args = (G3[:, t], hp[:, t], cprev, w_hh, b_ih, b_hh)
        rg, rc, rh = R.ref64(R.lstm_step, *args)
        cg, cc, ch = R.fp32_chain(R.lstm_step, *args)
        R.assert_close(gates.cpu()[:, t], rg, cg, gmag, f"gates {variant} t={t}")
        R.assert_close(ck[:, t], rc, cc, 1.0, f"c {variant} t={t}")
        R.assert_close(h_out.cpu()[:, t], rh, ch, 1.0, f"h_out {variant} t={t}")

    # backward from the contract's own gates and c (the CPU fp32 chain of the whole recurrence): the exact float64 chain is
    # the reference, the fp32 chain that stores every step's dG in the dtype is the yardstick
    _, cg, cc = R.lstm_recurrence(G.float(), w_hh.float(), b_ih, b_hh, B, T, h_dtype=None if dtype == torch.float32 else dtype)
    cg, cc = cg.detach().contiguous(), cc.detach().contiguous()
    with guarded(dvt.ops):
        dG = dvt.ops.lstm_seq_bwd(dev(w_hh), dev(cg), dev(cc), dev(dh_seq), dev(dh_last))
    torch.cuda.synchronize()
    ref = R.ref64(R.lstm_bwd_chain, w_hh, cg, cc, dh_seq, dh_last)
    chain = R.fp32_chain(R.lstm_bwd_chain, w_hh, cg, cc, dh_seq, dh_last, store_dtype=None if dtype == torch.float32 else dtype)
    mag = max(float(t.double().abs().max()) for t in (dh_seq, dh_last) if t is not None)
    R.assert_close(dG.cpu(), ref, chain, mag, f"dG {variant}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_forward_step_k_loop_sums_every_group_once(dvt, dtype):
    """step 0 leaves h_0 = +-tau at one unit of every 8-wide group (tau = tanh(1) in the dtype) and exactly 0 elsewhere;
    step 1 then sums tau * (+-1) over the groups: gates[:, 1] = act(tau n) with the integer n of rowwise_ref.kstep_operands"""
    from tests import rowwise_ref as R
    B, H = R.KSTEP_B, R.KSTEP_H
    G, w_hh, n = R.kstep_operands(dtype)
    h_out, h_prev, gates, c, _ = _seq_fwd_poisoned(dvt, G.cuda(), w_hh.cuda(), None, None, B, 2, False)
    torch.cuda.synchronize()
    h0 = h_out[:, 0].cpu().double()
    taus = h0.abs()[h0 != 0].unique()
    assert taus.numel() == 1, taus
    tau = float(taus)
    want = torch.tensor(math.tanh(1.0), dtype=torch.float64).to(dtype)
    got = torch.tensor(tau, dtype=torch.float64).to(dtype)
    if dtype == torch.float32:
        assert abs(tau - math.tanh(1.0)) <= 2.0 ** -24                      # one fp32 ulp at 0.76
    else:
        assert abs(int(R.ordinal(got.reshape(1))) - int(R.ordinal(want.reshape(1)))) <= 1
    assert torch.equal((h0 != 0).reshape(B, H // 8, 8).sum(2), torch.ones(B, H // 8, dtype=torch.int64))
    err = float((gates[:, 1].cpu().double() - R.kstep_gates(n, tau)).abs().max())
    assert err <= KSTEP_TOL, err
