"""tests/layernorm_ref.py checked on the CPU: its float64 statements against torch's own layer_norm / cross_entropy (with
autograd), the inputs of tests/test_gpu_layernorm.py against the rule they are judged by, and the rule against the errors
it is there to catch."""
import math

import pytest
import torch
import torch.nn.functional as TF

from tests import layernorm_ref as LR
from tests import rowwise_ref as R

D64 = torch.float64


def _case(n0, n1, d, seed, constant_row=None):
    g = LR.gen(seed)
    x = LR.randn((n0 * n1, d), D64, g, 1.5, 0.5)
    if constant_row is not None:
        x[constant_row] = 3.0
    gamma, beta = (t.double() for t in LR.ln_params(d, g))
    return g, x, gamma, beta


@pytest.mark.parametrize("d", [8, 40, 520])
def test_ln_fwd_is_torch_layer_norm(d):
    _, x, gamma, beta = _case(5, 1, d, 1, constant_row=3)
    y, mean, rstd = LR.ln_fwd(x, gamma, beta, LR.EPS)
    torch.testing.assert_close(y, TF.layer_norm(x, (d,), gamma, beta, LR.EPS), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(mean, x.mean(1), rtol=1e-14, atol=0)
    torch.testing.assert_close(rstd, 1.0 / torch.sqrt(x.var(1, unbiased=False) + LR.EPS), rtol=1e-12, atol=0)
    assert float(rstd[3]) == 1.0 / math.sqrt(LR.EPS) and torch.equal(y[3], beta)          # the constant row
    assert LR.EPS == float(torch.tensor(1e-5, dtype=torch.float32))


@pytest.mark.parametrize("n1", [1, 5])
def test_ln_bwd_is_autograd_with_the_added_operands(n1):
    """dy_first enters dy of row (i0, 0) and with it dgamma and dbeta; dx_first and dx_add enter dx only"""
    n0, d = 3, 40
    g, x, gamma, beta = _case(n0, n1, d, 2, constant_row=1)
    dy, add = LR.randn((n0 * n1, d), D64, g), LR.randn((n0 * n1, d), D64, g)
    dyf, dxf = LR.randn((n0, d), D64, g), LR.randn((n0, d), D64, g)
    _, mean, rstd = LR.ln_fwd(x, gamma, beta, LR.EPS)
    dy0 = dy.clone()
    for use_dyf, use_dxf, use_add in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        dy_tot = dy.clone()
        if use_dyf:
            dy_tot.view(n0, n1, d)[:, 0] += dyf
        TF.layer_norm(xr, (d,), gr, br, LR.EPS).backward(dy_tot)
        want_dx = xr.grad.clone()
        if use_add:
            want_dx += add
        if use_dxf:
            want_dx.view(n0, n1, d)[:, 0] += dxf
        dx, dg, db = LR.ln_bwd(dy, x, gamma, mean, rstd, add if use_add else None, dyf if use_dyf else None,
                               dxf if use_dxf else None, n1=n1)
        torch.testing.assert_close(dx, want_dx, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(dg, gr.grad, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(db, br.grad, rtol=1e-12, atol=1e-12)
    assert torch.equal(dy, dy0)                                                        # (ln_bwd leaves its operands alone)


def test_ln_bwd_works_from_the_statistics_it_is_handed():
    """rounded statistics change the result: the backward does not recompute them"""
    g, x, gamma, beta = _case(4, 1, 40, 3)
    dy = LR.randn((4, 40), D64, g)
    _, mean, rstd = LR.ln_fwd(x, gamma, beta, LR.EPS)
    a = LR.ln_bwd(dy, x, gamma, mean, rstd)[0]
    b = LR.ln_bwd(dy, x, gamma, mean.float().double(), rstd.float().double())[0]
    assert not torch.equal(a, b) and float((a - b).abs().max()) < 1e-6
    m32, r32 = LR.stats32(x, gamma.float(), beta.float())
    assert m32.dtype == torch.float32 and torch.equal(m32, mean.float()) and torch.equal(r32, rstd.float())


@pytest.mark.parametrize("M,C", [(1, 1), (17, 65), (33, 305)])
def test_ce_labels_is_torch_cross_entropy(M, C):
    logits, labels = LR.ce_case(M, C, D64, LR.gen(M + C))
    if M > 1:
        assert bool((labels[1::16] == -100).all()) and int((labels == -100).sum()) == len(labels[1::16]) + 1
    xr = logits.clone().requires_grad_(True)
    want = TF.cross_entropy(xr, labels, ignore_index=-100)
    loss, lse, count = LR.ce_labels(logits, labels, -100)
    torch.testing.assert_close(loss, want.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(lse, torch.logsumexp(logits, 1), rtol=0, atol=0)
    assert float(count) == float((labels != -100).sum())
    gloss = torch.tensor([1.7], dtype=D64)
    want.backward(gloss[0])
    d = LR.ce_labels_bwd(logits, labels, lse, count, gloss, -100)
    torch.testing.assert_close(d, xr.grad, rtol=1e-12, atol=1e-14)
    assert bool((d[labels == -100] == 0).all())


def test_ce_labels_edges():
    logits, labels = LR.ce_case(17, 65, D64, LR.gen(5), ignored="all")
    loss, lse, count = LR.ce_labels(logits, labels, -100)
    assert math.isnan(float(loss)) and float(count) == 0.0
    assert math.isnan(float(TF.cross_entropy(logits, labels, ignore_index=-100)))         # torch's mean over no rows
    d = LR.ce_labels_bwd(logits, labels, lse, count, torch.tensor([1.7], dtype=D64), -100)
    assert bool((d == 0).all())                                                         # although gloss / count is infinite
    logits, labels = LR.ce_case(17, 65, D64, LR.gen(6))
    labels[5] = 65
    loss, lse, count = LR.ce_labels(logits, labels, -100)
    assert math.isnan(float(loss)) and float(count) == float((labels != -100).sum())
    d = LR.ce_labels_bwd(logits, labels, lse, count, torch.tensor([1.7], dtype=D64), -100)
    assert bool(torch.isnan(d[5]).all()) and bool((d[labels == -100] == 0).all())
    rest = [r for r in range(17) if r != 5 and labels[r] != -100]
    assert bool(torch.isfinite(d[rest]).all()) and bool((d[rest] != 0).all())


# ---------------------------------------------------------------- the chosen inputs against the rule
def _chosen_inputs():
    """(tag, dtype, x, dy, d) of every kind of content tests/test_gpu_layernorm.py uses, at the widths it uses them"""
    from tests import test_gpu_layernorm as T
    for name in T.DT:
        dtype = R.DTYPES[name]
        for d in T.WIDTHS:
            g = LR.gen(d)
            yield f"ordinary {name} d={d}", dtype, T._x((9, d), name, g), LR.randn((9, d), dtype, g), d
        for d in (8, 520, 4096):
            g = LR.gen(d)
            yield f"offset {name} d={d}", dtype, LR.offset_rows(9, d, dtype, g), LR.randn((9, d), dtype, g), d
        for d in (8, 1024):
            yield f"constant {name} d={d}", dtype, LR.constant_rows(1, d, dtype), LR.randn((1, d), dtype, LR.gen(d)), d
    for d in (40, 2056):
        g = LR.gen(d)
        yield f"fp16 top d={d}", torch.float16, LR.fp16_top_rows(5, d, g), LR.fp16_top_rows(5, d, g), d


def test_the_fp32_chain_is_finite_and_inside_the_rule_on_every_chosen_input():
    """what the rule asks of a kernel, asked of the plain fp32 evaluation rounded once to the output type"""
    for tag, dtype, x, dy, d in _chosen_inputs():
        gamma, beta = LR.ln_params(d, LR.gen(d + 1))
        assert bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(dy.float()).all()), tag
        y, mean, rstd = R.fp32_chain(LR.ln_fwd, x, gamma, beta)
        assert all(bool(torch.isfinite(t).all()) for t in (y, mean, rstd)), tag
        LR.check_fwd(y.to(dtype), mean, rstd, x, gamma, beta, tag)
        m32, r32 = LR.stats32(x, gamma, beta)
        dx, dg, db = R.fp32_chain(LR.ln_bwd, dy, x, gamma, m32, r32)
        assert all(bool(torch.isfinite(t).all()) for t in (dx, dg, db)) and bool(torch.isfinite(dx.to(dtype).float()).all()), tag
        LR.check_bwd(dx.to(dtype), dg, db, dy, x, gamma, m32, r32, tag)
        if tag.startswith("offset"):
            # the rows are what they are meant to be: a one-pass fp32 variance is lost, no row became constant
            x32 = x.float()
            one_pass = (x32 * x32).mean(1) - x32.mean(1) ** 2
            two_pass = x.double().var(1, unbiased=False)
            assert bool((two_pass > 0).all()) and float(x.double().mean(1).min()) > 99.0
            assert len({tuple(r.tolist()) for r in x32}) == x32.shape[0], tag
            if dtype != torch.bfloat16:                  # (bf16: see offset_rows)
                assert float(((one_pass.double() - two_pass).abs() / two_pass).max()) > 0.02, tag
        if tag.startswith("constant"):
            assert float(rstd[0]) == float((1.0 / torch.sqrt(torch.tensor(LR.EPS, dtype=D64))).float()), tag


# ---------------------------------------------------------------- the rule bites
def _fp32_case(rows, d, seed):
    g = LR.gen(seed)
    gamma, beta = LR.ln_params(d, g)
    x = LR.randn((rows, d), torch.float32, g, 1.5, 0.5)
    dy = LR.randn((rows, d), torch.float32, g)
    return x, dy, gamma, beta


@pytest.mark.parametrize("rows,d", [(9, 40), (3, 4096)])
def test_one_element_of_the_last_row_off_by_8_ulps_is_rejected(rows, d):
    """the error of a wrong last row of a second trip, or of one wrong vector: on the best fp32 output there is (the
    float64 result rounded), the largest element of the last row moved by 8 fp32 ulps of its own magnitude.  (The budget
    there is 4 to 7 such ulps for y, 2 to 5 for rstd and 4 to 6 for dx at these shapes; the mean is judged in ulps of the
    largest |x_j| of its row, and moved by 8 of those.)"""
    x, dy, gamma, beta = _fp32_case(rows, d, 40 + d)
    mean, rstd = LR.stats32(x, gamma, beta)
    fwd = [t.float() for t in R.ref64(LR.ln_fwd, x, gamma, beta)]
    bwd = [t.float() for t in R.ref64(LR.ln_bwd, dy, x, gamma, mean, rstd)]
    LR.check_fwd(*fwd, x, gamma, beta, "unperturbed")
    LR.check_bwd(*bwd, dy, x, gamma, mean, rstd, "unperturbed")

    def off(t):
        t = t.clone()
        last = t[-1] if t.dim() == 2 else t[-1:]
        j = int(last.abs().argmax())
        last[j] += 8 * float(R.ulp32(last[j]))
        return t

    for k, what in enumerate(("y", "mean", "rstd")):
        if what == "mean":
            continue                                    # (judged in ulps of max |x_j| of its row, not of its own size: below)
        out = list(fwd)
        out[k] = off(out[k])
        with pytest.raises(AssertionError, match=f"^{what} "):
            LR.check_fwd(*out, x, gamma, beta, "perturbed")
    out = list(fwd)
    out[1] = out[1].clone()
    out[1][-1] += 8 * float(R.ulp32(x[-1].abs().max()))
    with pytest.raises(AssertionError, match="^mean "):
        LR.check_fwd(*out, x, gamma, beta, "perturbed")
    with pytest.raises(AssertionError, match="^dx "):
        LR.check_bwd(off(bwd[0]), bwd[1], bwd[2], dy, x, gamma, mean, rstd, "perturbed")


@pytest.mark.parametrize("rows,d", [(9, 40), (4097, 8)])
def test_a_dgamma_column_short_of_one_partial_row_is_rejected(rows, d):
    """workgroup b of the backward sums rows 4 b .. 4 b + 3 (and, past the cap of 1,024 workgroups, 4096 rows further on)
    into partial row b: a reduce that leaves one partial row out of one column, every column and dbeta in turn"""
    x, dy, gamma, beta = _fp32_case(rows, d, 50 + d)
    mean, rstd = LR.stats32(x, gamma, beta)
    dx, dg, db = [t.float() for t in R.ref64(LR.ln_bwd, dy, x, gamma, mean, rstd)]
    LR.check_bwd(dx, dg, db, dy, x, gamma, mean, rstd, "unperturbed")
    _, xh, _, _, _ = LR.ln_bwd_terms(dy.double(), x.double(), gamma.double(), mean.double(), rstd.double())
    blocks = (torch.arange(rows) // 4) % 1024
    for b in (0, int(blocks[-1])):                      # the first partial row, and the one the last row goes into
        part_g = (dy.double() * xh)[blocks == b].sum(0)
        part_b = dy.double()[blocks == b].sum(0)
        for c in range(d):
            short = dg.clone()
            short[c] = float(dg[c].double() - part_g[c])
            with pytest.raises(AssertionError, match="^dgamma "):
                LR.check_bwd(None, short, db, dy, x, gamma, mean, rstd, f"column {c} short of partial row {b}")
            short = db.clone()
            short[c] = float(db[c].double() - part_b[c])
            with pytest.raises(AssertionError, match="^dbeta "):
                LR.check_bwd(None, dg, short, dy, x, gamma, mean, rstd, f"column {c} short of partial row {b}")
