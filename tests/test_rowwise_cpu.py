"""CPU checks of tests/rowwise_ref.py: the float64 references equal the torch modules they restate, the edge inputs are on
the edge, the tolerance rule rejects what it should, and the k-step operands of the LSTM forward step see every fault of
its K loop (section "k-step" below has the two measured numbers the GPU tolerance sits between)."""
import math

import pytest
import torch
import torch.nn.functional as TF
from torch import nn

from tests import contrastive_ref as CR
from tests import rowwise_ref as R

D64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- references against the modules they restate
@pytest.mark.parametrize("eps", [1e-8, 1e-12])
def test_cosine_and_l2norm_equal_torch(eps):
    g = _gen(1)
    for D in (1, 7, 65):
        x = R.l2norm_edge_rows(D, torch.float32, eps, g).double()
        y = torch.flip(x, [0]) + 0.5 * torch.randn(x.shape, generator=g, dtype=D64) * x.abs().max(1, keepdim=True).values
        assert torch.allclose(R.cosine_rows(x, y, eps), nn.CosineSimilarity(dim=1, eps=eps)(x, y), rtol=1e-12, atol=0)
        assert torch.allclose(R.l2norm_rows(x, eps), TF.normalize(x, dim=1, eps=eps), rtol=1e-14, atol=0)
        dy = torch.randn(x.shape, generator=g, dtype=D64)
        dx = R.l2norm_rows_bwd(x, dy, eps)
        clamped = x.norm(dim=1) < eps
        assert clamped[0] and clamped[1]
        assert torch.equal(dx[clamped], dy[clamped] / eps)                                  # torch gives dy / eps there
        from_y = R.l2norm_rows_bwd_from_y(R.l2norm_rows(x, eps), R.l2norm_inv(x, eps), dy, eps)
        scale = (R.l2norm_inv(x, eps).unsqueeze(1) * dy.abs()).max(1, keepdim=True).values    # dx cancels to 0 where D = 1
        assert ((from_y - dx).abs() <= 1e-12 * scale).all()


def test_cosine_small_norm_pair_is_where_the_two_clamps_part():
    a, b = R.cosine_small_norm_pair(torch.float32)
    a, b = a.double(), b.double()
    eps = 1e-8
    assert float(a.norm()) > eps and float(b.norm()) > eps and float(a.norm() * b.norm()) < eps
    torch_says = float(nn.CosineSimilarity(dim=1, eps=eps)(a, b))
    assert abs(torch_says - 0.96) < 1e-6 and abs(float(R.cosine_rows(a, b, eps)) - torch_says) < 1e-12
    product_clamp = float((a * b).sum() / max(float(a.norm() * b.norm()), eps))             # what the kernel used to do
    assert abs(product_clamp - 0.0024) < 1e-6


def test_gate_contrastive_and_losses_equal_torch():
    g = _gen(2)
    x, x1 = torch.randn(5, 12, generator=g, dtype=D64), torch.randn(5, 12, generator=g, dtype=D64)
    assert torch.allclose(R.gate(x, x + x1), TF.glu(torch.cat((x, x + x1), -1), -1), rtol=1e-14, atol=0)
    dy = torch.randn(5, 12, generator=g, dtype=D64)
    xa, xb = x.clone().requires_grad_(True), (x + x1).clone().requires_grad_(True)
    TF.glu(torch.cat((xa, xb), -1), -1).backward(dy)
    da, db = R.gate_bwd(x, x + x1, dy)
    assert torch.allclose(da, xa.grad, rtol=1e-13, atol=0) and torch.allclose(db, xb.grad, rtol=1e-13, atol=1e-300)

    for T in (0.1, 0.5):
        zi, zj = torch.randn(3, 8, generator=g, dtype=D64), torch.randn(3, 8, generator=g, dtype=D64)
        reps = torch.cat([zi, zj], 0)
        sim = TF.cosine_similarity(reps.unsqueeze(1), reps.unsqueeze(0), dim=2)
        loss, lse, row = R.contrastive_rows(sim, T)
        assert abs(float(loss) - float(CR.ntxent(zi, zj, T))) < 1e-12
        assert torch.allclose(row.mean(), loss)

    z = torch.randn(40, generator=g, dtype=D64) * 10
    z[:2] = 0.0                                                                              # the kink of max(z, 0) and |z|
    y = (torch.rand(40, generator=g) < 0.4).double()
    assert abs(float(R.bce_logits(z, y)) - float(TF.binary_cross_entropy_with_logits(z, y))) < 1e-14
    zr = z.clone().requires_grad_(True)
    TF.binary_cross_entropy_with_logits(zr, y).backward(torch.tensor(1.7, dtype=D64))
    assert torch.allclose(R.bce_logits_bwd(z, y, torch.tensor([1.7], dtype=D64)), zr.grad, rtol=1e-12, atol=1e-16)   # (s - y cancels)
    assert abs(float(R.sigmoid_bce(z, y)) - float(nn.BCELoss()(torch.sigmoid(z), y))) < 1e-13
    zr = z.clone().requires_grad_(True)
    nn.BCELoss()(torch.sigmoid(zr), y).backward(torch.tensor(0.3, dtype=D64))
    assert torch.allclose(R.sigmoid_bce_bwd(z, y, torch.tensor([0.3], dtype=D64)), zr.grad, rtol=1e-10, atol=1e-16)

    st, te = R.ce_case(4, 130, torch.float32, g)
    st, te = st.double(), te.double()
    assert abs(float(R.ce_argmax(st, te)) - float(TF.cross_entropy(st, te.argmax(1)))) < 1e-13
    sr = st.clone().requires_grad_(True)
    TF.cross_entropy(sr, te.argmax(1)).backward(torch.tensor(2.0, dtype=D64))
    assert torch.allclose(R.ce_argmax_bwd(st, te, torch.tensor([2.0], dtype=D64)), sr.grad, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("kind,module", [(R.ACT_GELU, nn.GELU()), (R.ACT_RELU, nn.ReLU()), (R.ACT_SIGMOID, nn.Sigmoid())])
def test_activations_equal_torch(kind, module):
    x = R.elementwise_values(300, torch.float32, _gen(3)).double()
    dy = torch.randn(300, generator=_gen(4), dtype=D64)
    assert torch.allclose(R.act(x, kind), module(x), rtol=1e-13, atol=1e-300)
    xr = x.clone().requires_grad_(True)
    module(xr).backward(dy)
    assert torch.allclose(R.act_bwd(x, dy, kind), xr.grad, rtol=1e-12, atol=1e-300)


def test_data_movement_references():
    g = _gen(5)
    x = torch.randn(3, 17, 8, generator=g, dtype=D64)
    assert torch.allclose(R.mean_rows(x), x.mean(1), rtol=1e-14, atol=0)
    assert torch.equal(R.mean_rows(x, 0.5), x.sum(1) * 0.5)
    xr = x.clone().requires_grad_(True)
    dout = torch.randn(3, 8, generator=g, dtype=D64)
    xr.mean(1).backward(dout)
    assert torch.allclose(R.mean_rows_bwd(dout, 17), xr.grad, rtol=1e-14, atol=0)
    src = torch.randn(2, 5, 4, 8, generator=g, dtype=D64)
    tok = torch.randn(8, generator=g, dtype=D64)
    assert torch.equal(R.rows_gather(src, None), src[:, :, 0])
    assert torch.equal(R.rows_gather(src, tok)[:, 0], tok.expand(2, 8)) and torch.equal(R.rows_gather(src, tok)[:, 1:], src[:, :, 0])
    # token assembly: out[s] = cat(cls, emb[s]) + pos[s % T, :n + 1]
    S, T, n, d, rows = 6, 3, 4, 8, 7
    emb = torch.randn(S * n, d, generator=g, dtype=D64, requires_grad=True)
    cls = torch.randn(d, generator=g, dtype=D64, requires_grad=True)
    pos = torch.randn(T, rows, d, generator=g, dtype=D64, requires_grad=True)
    out = torch.cat((cls.expand(S, 1, d), emb.reshape(S, n, d)), 1) + pos[:, :n + 1].repeat(S // T, 1, 1)
    dout = torch.randn(S, n + 1, d, generator=g, dtype=D64)
    out.backward(dout)
    demb, dcls, dpos = R.tokens_assemble_bwd(dout, T, rows)
    assert torch.equal(demb, emb.grad) and torch.allclose(dcls, cls.grad) and torch.allclose(dpos, pos.grad)
    assert torch.equal(dpos[:, n + 1:], torch.zeros(T, rows - n - 1, d, dtype=D64))
    dst = torch.full((4,), math.nan, dtype=D64)
    assert torch.equal(R.axpby(dst, torch.ones(4, dtype=D64), 2.0, 0.0), torch.full((4,), 2.0, dtype=D64))
    assert torch.isnan(R.axpby(dst, torch.ones(4, dtype=D64), 2.0, 1.0)).all()


# ---------------------------------------------------------------- the edge inputs are on the edge
@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("eps", [1e-8, 1e-12])
def test_l2norm_edge_rows_are_on_the_edge(name, eps):
    dtype = R.DTYPES[name]
    for D in (1, 7, 63, 64, 65, 200):
        x = R.l2norm_edge_rows(D, dtype, eps, _gen(D))
        nrm = x.double().norm(dim=1)
        assert float(nrm[0]) == 0.0
        if dtype != torch.float16:                                   # fp16's smallest subnormal (6e-8) is above both eps
            assert 0.0 < float(nrm[1]) < eps, (D, float(nrm[1]))
            assert eps < float(nrm[2]) < 8 * eps
        else:
            assert float(nrm[1]) == 0.0
            big = x[4].double().abs()
            assert float(big.min()) > 2.5e4 and float((x[4].float() ** 2).min()) > 65504.0   # squares overflow fp16
            assert torch.isinf((x[4] * x[4])).all()
        assert float(nrm[3]) > 1e-3 and int((x[5] != 0).sum()) == 1


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
def test_elementwise_values_hold_the_saturated_logits(name):
    dtype = R.DTYPES[name]
    x = R.elementwise_values(9, dtype, _gen(0)).double()
    want = [0.0, -0.0, 20.0, -20.0, 100.0, -100.0] + ([6.0e4, -6.0e4] if dtype == torch.float16 else [])
    assert x[:len(want)].tolist() == want and math.copysign(1.0, float(x[1])) == -1.0
    assert float(torch.sigmoid(torch.tensor(100.0))) == 1.0 and float(torch.sigmoid(torch.tensor(-100.0, dtype=torch.float32))) < 1e-38
    assert [len(R.elementwise_values(n, dtype, _gen(0))) for n in (1, 7, 8, 9)] == [1, 7, 8, 9]
    rest = R.elementwise_values(2051, dtype, _gen(1)).double()[8:]
    assert float(rest.abs().max()) <= 3.0


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
def test_ce_ties_straddle_lanes_and_one_row_is_all_minus_inf(name):
    dtype = R.DTYPES[name]
    for rows in (1, 3, 4, 9):
        for C in (1, 5, 64, 65, 400):
            st, te = R.ce_case(rows, C, dtype, _gen(rows * 1000 + C))
            t = te.double()
            for r in range(rows):
                if rows >= 3 and r == 1:
                    assert torch.isinf(t[r]).all() and (t[r] < 0).all() and r != rows - 1
                    assert int(t[r].argmax()) == 0                                   # torch's answer for such a row
                    continue
                top = (t[r] == t[r].max()).nonzero().flatten().tolist()
                if C >= 3:
                    assert len(top) == 2 and int(t[r].argmax()) == top[0], (rows, C, r, top)
            if C == 400 and rows >= 4:
                pairs = {tuple((te[r].double() == te[r].double().max()).nonzero().flatten().tolist()) for r in range(rows) if r != 1}
                assert {(5, 64), (3, 67), (6, 70)} <= pairs or rows == 4
                assert any(i % 64 > j % 64 for i, j in pairs)                        # first maximum in the higher lane
                assert any(i % 64 == j % 64 for i, j in pairs)                       # both in one lane
            if C == 65:
                assert tuple((t[0] == t[0].max()).nonzero().flatten().tolist()) == (5, 64)


def test_contrastive_sim_has_the_large_logit():
    for M in (2, 4, 6, 130, 258):
        for T in (0.1, 0.5):
            sim = R.contrastive_sim(M, T, _gen(M))
            assert sim.shape == (M, M) and abs(float(sim[0, 1 % M]) / T - 1000.0) < 1e-3
            loss, lse, row = R.ref64(R.contrastive_rows, sim, temperature=T)
            assert torch.isfinite(lse).all() and torch.isfinite(loss)
            naive = torch.exp(sim[0].float() / T)                                      # what must not be formed in fp32
            assert torch.isinf(naive).any()


# ---------------------------------------------------------------- the tolerance rule
def test_tolerance_rule_accepts_a_neighbour_and_rejects_two_steps():
    g = _gen(7)
    for dtype in (torch.bfloat16, torch.float16):
        x = R.elementwise_values(500, dtype, g)
        ref = R.ref64(R.act, x, kind=R.ACT_SIGMOID)
        chain = R.fp32_chain(R.act, x, kind=R.ACT_SIGMOID)
        exact = ref.to(dtype)
        R.assert_close(exact, ref, chain, x.double().abs())
        R.assert_close(R.fp32_chain(R.act, x, kind=R.ACT_SIGMOID, out_dtype=dtype), ref, chain, x.double().abs())
        mid = (exact.double() > 0.3) & (exact.double() < 0.7)
        one = torch.where(mid, torch.nextafter(exact, torch.ones_like(exact)), exact)
        R.assert_close(one, ref, chain, x.double().abs())
        three = torch.nextafter(torch.nextafter(one, torch.ones_like(one)), torch.ones_like(one))
        three = torch.where(mid, three, exact)
        with pytest.raises(AssertionError):
            R.assert_close(three, ref, chain, x.double().abs())
    x = R.elementwise_values(500, torch.float32, g)
    ref = R.ref64(R.act, x, kind=R.ACT_SIGMOID)
    chain = R.fp32_chain(R.act, x, kind=R.ACT_SIGMOID)
    R.assert_close(chain, ref, chain, x.double().abs())
    off = chain.clone()
    off[20] += 2e-6                                                  # ~30 fp32 ulps of a sigmoid near 0.5
    with pytest.raises(AssertionError):
        R.assert_close(off, ref, chain, x.double().abs())
    with pytest.raises(AssertionError):
        R.assert_close(torch.full_like(chain, math.nan), ref, chain, x.double().abs())


def test_one_huge_element_buys_no_slack_for_the_small_ones():
    ref = torch.tensor([1.0e12, 0.5], dtype=D64)
    chain = torch.tensor([1.0e12 + 65536.0, 0.5], dtype=D64)          # one fp32 ulp off at 1e12
    E = R.budget(ref, chain, torch.tensor([1.0, 1.0]))
    assert float(E[0]) >= 65536.0 and float(E[1]) < 1e-6


# ---------------------------------------------------------------- k-step: the LSTM forward step's K loop
# Measured here (CPU, float64): the smallest change any fault makes to its most affected gate is KSTEP_MARGIN; the
# reference's own fp32 evaluation is off by at most KSTEP_FP32_ERR.  tests/test_gpu_lstm.py asserts KSTEP_TOL.
KSTEP_MARGIN = 0.64          # measured 0.6420 (fp32 tau), 0.6421 (bf16 / fp16 tau)
KSTEP_FP32_ERR = 3.5e-8      # measured 1.2e-8 (fp32 tau), 3.5e-8 (bf16 / fp16 tau)
KSTEP_TOL = 1e-4             # 2,800 x the fp32 error, 6,400 x inside the margin


def _tau(dtype):
    return float(torch.tensor(math.tanh(1.0), dtype=D64).to(dtype).double())


def test_kstep_operands_are_what_the_docstring_says():
    for dtype in R.DTYPES.values():
        G, w, n = R.kstep_operands(dtype)
        B, H = R.KSTEP_B, R.KSTEP_H
        assert B % 16 == 1 and H % 16 == 0 and H % 32 == 16 and H // 32 >= 5           # ragged tile; wave 1's half chunk
        assert torch.equal(G.double(), G.double().round()) and float(G.double().abs().max()) == 200.0
        wq = w.double().reshape(4 * H, H // 8, 8)
        assert torch.equal(wq, wq[:, :, :1].expand_as(wq)) and set(wq.unique().tolist()) == {-1.0, 1.0}
        assert int(n.abs().max()) <= 3 and set(n.unique().tolist()) == {-2, 0, 2}
        h, gates, c = R.lstm_recurrence(G.double(), w.double(), None, None, B, 2)
        h0 = h[:, 0].reshape(B, H // 8, 8)
        is_open = h0.abs() > 0.5
        assert torch.equal(is_open.sum(2), torch.ones(B, H // 8, dtype=torch.int64))   # one open unit per 8-wide group
        where = is_open.double().argmax(2)
        assert not torch.equal(where[0], where[1])                                       # at a place that depends on the row
        assert float((h0[~is_open]).abs().max()) < 1e-80                                 # exactly 0 in fp32
        assert float((h0[is_open].abs() - math.tanh(1.0)).abs().max()) < 1e-12
        # fp32 saturation is exact: sigmoid(40) = 1, tanh(40) = 1, sigmoid(-200) = 0
        f = torch.float32
        assert float(torch.sigmoid(torch.tensor(40.0, dtype=f))) == 1.0 and float(torch.tanh(torch.tensor(40.0, dtype=f))) == 1.0
        assert float(torch.sigmoid(torch.tensor(-200.0, dtype=f))) == 0.0
        assert float((gates[:, 1] - R.kstep_gates(n, math.tanh(1.0))).abs().max()) < 1e-12


def test_kstep_operands_see_every_fault_of_the_k_loop():
    base, faults = R.kstep_faulty_sums()
    Q = R.KSTEP_H // 8
    assert len(faults) == 2 * (Q + (Q + 3) // 4 + 4) + Q
    for dtype in R.DTYPES.values():
        tau = _tau(dtype)
        good = R.kstep_gates(base, tau)
        margins = {name: float((R.kstep_gates(n, tau) - good).abs().max()) for name, n in faults.items()}
        worst = min(margins, key=margins.get)
        assert margins[worst] >= KSTEP_MARGIN, (worst, margins[worst])
        s32 = torch.tensor(tau, dtype=torch.float32) * base.float()
        H = base.shape[1] // 4
        g32 = torch.sigmoid(s32)
        g32[:, 2 * H:3 * H] = torch.tanh(s32[:, 2 * H:3 * H])
        err = float((g32.double() - good).abs().max())
        assert err <= KSTEP_FP32_ERR
        assert 100 * err <= KSTEP_TOL <= margins[worst] / 100


# ---------------------------------------------------------------- the LSTM statements
def test_lstm_statements_equal_torch_and_each_other():
    g = _gen(21)
    B, T, Fd, H = 5, 4, 12, 16
    lstm = nn.LSTM(Fd, H, 1, batch_first=True).double()
    x = torch.randn(B, T, Fd, generator=g, dtype=D64)
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0))
    G = x.reshape(B * T, Fd) @ w_ih.T
    h, gates, c = R.lstm_recurrence(G, w_hh, b_ih, b_hh, B, T)
    out, (hn, cn) = lstm(x)
    assert torch.allclose(h, out, rtol=1e-12, atol=1e-14) and torch.allclose(c[:, -1], cn[0], rtol=1e-12, atol=1e-14)
    gt, ct, ht = R.lstm_step(G.reshape(B, T, -1)[:, 2], h[:, 1], c[:, 1], w_hh, b_ih, b_hh)       # one step from a carried state
    assert torch.equal(gt, gates[:, 2]) and torch.equal(ct, c[:, 2]) and torch.equal(ht, h[:, 2])
    ds, dl = torch.randn(B, T, H, generator=g, dtype=D64), torch.randn(B, H, generator=g, dtype=D64)
    for a, b in ((ds, dl), (ds, None), (None, dl)):                                                 # the explicit backward chain
        assert torch.allclose(R.lstm_bwd_chain(w_hh, gates, c, a, b), R.lstm_dG(G, w_hh, b_ih, b_hh, B, T, a, b), rtol=1e-11, atol=1e-14)
    stored = R.lstm_bwd_chain(w_hh, gates, c, ds, dl, store_dtype=torch.float16)
    assert torch.equal(stored, stored.half().double()) and not torch.equal(stored, R.lstm_bwd_chain(w_hh, gates, c, ds, dl))
    # the fp16 restatement differs from the fp32 layer by 16-bit rounding only
    o16, l16, g16 = R.lstm_layer_restated(x.half(), w_ih.half(), w_hh.half(), b_ih.float(), b_hh.float(), ds, dl, torch.float16)
    assert torch.equal(o16, o16.half().float()) and torch.equal(l16, o16[:, -1])
    xs = x.half().float().requires_grad_(True)
    h32, _, _ = R.lstm_recurrence(xs.reshape(B * T, Fd) @ w_ih.half().float().T, w_hh.half().float(), b_ih.float(), b_hh.float(), B, T)
    ((h32 * ds.half().float()).sum() + (h32[:, -1] * dl.half().float()).sum()).backward()
    assert 0 < float((o16 - h32.detach()).norm() / h32.detach().norm()) < 2e-3
    assert 0 < float((g16["dx"] - xs.grad).norm() / xs.grad.norm()) < 4e-3
