"""tests/batchnorm_ref.py checked on the CPU: its float64 statements against torch's own batch_norm / max_pool2d (with
autograd), its builders against the properties tests/test_gpu_batchnorm.py relies on (sums exact below 2^24, no element of
a mask-recompute case inside the margin, no constant column), its mirrors against the text of csrc/conv.hip, and the judge
against the faults it is there to catch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import batchnorm_ref as B
from tests import rowwise_ref as R

D64 = torch.float64


def _nchw(t, N, H, W):
    return t.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---------------------------------------------------------------- the statements against torch in float64
@pytest.mark.parametrize("rows,C", [(2, 8), (37, 16), (300, 45)])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_bn_train_is_torch_batch_norm(rows, C, relu, res):
    g = B.gen(rows + C)
    x = B.feature_map(rows, C, D64, g)
    r = B.randn((rows, C), D64, g) if res else None
    gamma, beta = (t.double() for t in B.bn_params(C, g, both_signs=True))
    rm0, rv0 = torch.randn(C, generator=g, dtype=D64), torch.rand(C, generator=g, dtype=D64) + 0.5
    dy = B.randn((rows, C), D64, g)
    for momentum in (0.1, 1.0):
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        rr = None if r is None else r.clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        y = TF.batch_norm(xr, rm, rv, gr, br, True, momentum, B.EPS)
        y = y if rr is None else y + rr
        y = torch.relu(y) if relu else y
        y.backward(dy)
        mean, var, invstd = B.bn_stats(x, B.EPS)
        torch.testing.assert_close(B.bn_fwd(x, mean, invstd, gamma, beta, r, relu), y.detach(), rtol=1e-12, atol=1e-12)
        m2, i2, rm2, rv2 = B.stats_with_running(x, rm0, rv0, momentum, B.EPS)
        torch.testing.assert_close(rm2, rm, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(rv2, rv, rtol=1e-13, atol=1e-13)
        on = (y.detach() > 0).double() if relu else None
        dx, dz, dg, db = B.bn_bwd(dy, x, on, mean, invstd, gamma, True)
        torch.testing.assert_close(dx, xr.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(dg, gr.grad, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(db, br.grad, rtol=1e-12, atol=1e-12)
        if rr is not None:
            assert torch.equal(dz, rr.grad)
        if relu:                                        # the mask bytes carry the same decision
            assert torch.equal(B.mask_bits(B.mask_bytes(y.detach()), C), on) if C % 8 == 0 else True


def test_bn_eval_is_torch_batch_norm_in_eval_mode():
    rows, C = 37, 16
    g = B.gen(5)
    x, dy = B.feature_map(rows, C, D64, g), B.randn((rows, C), D64, g)
    gamma, beta = (t.double() for t in B.bn_params(C, g))
    rm, rv = torch.randn(C, generator=g, dtype=D64), torch.rand(C, generator=g, dtype=D64) + 0.5
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.relu(TF.batch_norm(xr, rm.clone(), rv.clone(), gr, br, False, 0.1, B.EPS))
    y.backward(dy)
    invstd = B.rsqrt_eps(rv, B.EPS)
    torch.testing.assert_close(B.bn_fwd(x, rm, invstd, gamma, beta, None, True), y.detach(), rtol=1e-12, atol=1e-12)
    dx, _, dg, db = B.bn_bwd(dy, x, (y.detach() > 0).double(), rm, invstd, gamma, False)
    torch.testing.assert_close(dx, xr.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dg, gr.grad, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(db, br.grad, rtol=1e-12, atol=1e-12)


def test_running_update_edges():
    """rows == 1: torch refuses to train on one value per channel; the statement is the update with no unbias factor.
    c_valid: the channels beyond it keep what they held."""
    C = 16
    g = B.gen(6)
    x = B.feature_map(1, C, D64, g)
    rm0, rv0 = torch.randn(C, generator=g, dtype=D64), torch.rand(C, generator=g, dtype=D64) + 0.5
    mean, invstd, rm, rv = B.stats_with_running(x, rm0, rv0, 0.1, B.EPS, c_valid=C - 3)
    assert torch.equal(mean, x[0]) and float(invstd[0]) == 1.0 / math.sqrt(B.EPS)
    torch.testing.assert_close(rm[:C - 3], 0.9 * rm0[:C - 3] + 0.1 * x[0, :C - 3], rtol=1e-14, atol=0)
    torch.testing.assert_close(rv[:C - 3], 0.9 * rv0[:C - 3], rtol=1e-14, atol=0)
    assert torch.equal(rm[C - 3:], rm0[C - 3:]) and torch.equal(rv[C - 3:], rv0[C - 3:])


def test_stats_from_partials_is_bn_stats():
    g = B.gen(7)
    x = B.feature_map(96, 8, D64, g)
    blocks = x.view(12, 8, 8)
    partial = torch.stack([blocks.sum(1), (blocks * blocks).sum(1)], 1)
    for a, b in zip(B.stats_from_partials(partial, 96, B.EPS), B.bn_stats(x, B.EPS)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)
    partial, rows, mean64, var64 = B.integer_partials(300, 8, B.gen(8))
    m, v, _ = B.stats_from_partials(partial[:300].double(), rows, B.EPS)
    assert torch.equal(m, mean64) and float((v - var64).abs().max()) < 1e-9 and bool(torch.isnan(partial[300:]).all())


def _torch_taps(idx, Ho, Wo, W, k, stride, pad):
    """max_pool2d's flat input indices [N, C, Ho, Wo] -> tap indices ki * k + kj"""
    h, w = idx // W, idx % W
    ki = h - (torch.arange(Ho).view(1, 1, Ho, 1) * stride - pad)
    kj = w - (torch.arange(Wo).view(1, 1, 1, Wo) * stride - pad)
    return ki * k + kj


@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2)])
@pytest.mark.parametrize("H,W", [(9, 11), (12, 16), (1, 5), (7, 2)])
@pytest.mark.parametrize("kind", ["random", "zeros", "negative"])
def test_maxpool_is_torch_max_pool2d(kind, H, W, k, stride, pad):
    """values, the first-maximum tap (on maps full of zeros as well) and the backward by autograd"""
    if H + 2 * pad < k or W + 2 * pad < k:
        return
    N, C = 2, 5
    g = B.gen(H * W + k)
    x = torch.randn(N * H * W, C, generator=g, dtype=D64)
    x = {"random": x, "zeros": x.clamp_min(0) * (x > 1.0), "negative": -0.5 - x.abs()}[kind]
    xr = _nchw(x, N, H, W).requires_grad_(True)
    want, idx = TF.max_pool2d(xr, k, stride, pad, return_indices=True)
    y, tap = B.maxpool_fwd(x, N, H, W, k, stride, pad)
    Ho, Wo = B.out_hw(H, W, k, stride, pad)
    assert (Ho, Wo) == tuple(want.shape[2:])
    assert torch.equal(y, _rows(want.detach()))
    assert torch.equal(tap.long(), _rows(_torch_taps(idx, Ho, Wo, W, k, stride, pad)))
    dy = B.randn(tuple(y.shape), D64, g)
    want.backward(_nchw(dy, N, Ho, Wo))
    geom = dict(N=N, H=H, W=W, k=k, stride=stride, pad=pad)
    torch.testing.assert_close(B.maxpool_bwd(dy, tap, **geom), _rows(xr.grad), rtol=1e-14, atol=1e-14)
    assert bool((B.maxpool_bwd_mag(dy, tap, **geom) >= B.maxpool_bwd(dy, tap, **geom).abs() / 9).all())


@pytest.mark.parametrize("H,W", [(2, 2), (9, 11), (12, 16)])
@pytest.mark.parametrize("relu", [True, False])
def test_stem_is_bn_relu_pool_with_autograd(H, W, relu):
    N, C = 3, 16
    g = B.gen(H + W)
    z = B.stem_map(N * H * W, C, D64, g)
    mean, invstd, gamma, beta = (t.double() for t in B.stem_params(C, g))
    zr, gr, br = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    y = (zr - mean) * invstd * gr + br
    y = torch.relu(y) if relu else y
    want, idx = TF.max_pool2d(_nchw(y, N, H, W), 3, 2, 1, return_indices=True)
    p, tap = B.stem_fwd(z, mean, invstd, gamma, beta, N, H, W, relu, D64)
    Ho, Wo = B.out_hw(H, W, 3, 2, 1)
    assert torch.equal(p, _rows(want.detach())) and torch.equal(tap.long(), _rows(_torch_taps(idx, Ho, Wo, W, 3, 2, 1)))
    dyp = B.randn(tuple(p.shape), D64, g)
    want.backward(_nchw(dyp, N, Ho, Wo))
    on = (y.detach() > 0).double() if relu else None
    dx, _, dg, db = B.stem_bwd(dyp, z, on, mean, invstd, gamma, tap, N, H, W, training=False)
    torch.testing.assert_close(dx, zr.grad, rtol=1e-12, atol=1e-12)          # (mean / invstd are constants here: eval)
    torch.testing.assert_close(dg, gr.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, br.grad, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- builder properties
def test_the_sequential_chain_is_sequential_fp32():
    """colsum in fp32 is the row-by-row sum with every addition rounded to fp32 (torch's own sum and cumsum of an fp32
    column accumulate in double on the CPU and would leave the chain all but exact)"""
    x = torch.randn(5000, 3, generator=B.gen(9))
    acc = np.zeros(3, dtype=np.float32)
    for r in x.numpy():
        acc = (acc + r).astype(np.float32)
    assert np.array_equal(B.colsum(x).numpy(), acc)
    assert torch.equal(B.colsum(x.double()), x.double().sum(0))
    assert float((B.colsum(x).double() - x.double().sum(0)).abs().max()) > 4 * float((x.sum(0).double() - x.double().sum(0)).abs().max())


def _integer_shapes():
    from tests import test_gpu_batchnorm as T
    shapes = {(rows, C) for C in T.WIDTHS for rows in T.row_counts(C)} | {T.SHORT_LAST} | set(T.BIG)
    shapes |= {(rows, C) for C in T.SCALAR_WIDTHS for rows in (1, 5, 300)} | {(5, T.MISALIGNED_C), (300, T.MISALIGNED_C)}
    return sorted(shapes)


def test_integer_maps_are_exact_in_every_dtype_and_below_2_to_24():
    """the builders assert it themselves; here: for every shape the GPU file uses, in every dtype, with the worst partial
    printed; and a map that breaks the bound is refused"""
    worst = 0.0
    for rows, C in _integer_shapes():
        for name, dtype in R.DTYPES.items():
            if rows * C > 1 << 20 and name != "bf16":
                continue                                # (the two 8 M maps: the same integers in every dtype)
            x = B.integer_map(rows, C, dtype, B.gen(rows + C))
            worst = max(worst, B.assert_partials_exact(x))
            if rows >= 2:
                assert not B.has_constant_column(x)
                assert float(x.double()[:, 0].mean()) >= 97.0 and 0.0 < float(x.double()[:, 0].var(unbiased=False)) <= 9.0
    print(f"largest partial of the integer maps: {worst} (2^24 = {2 ** 24})")
    assert 2 ** 23 < worst < 2 ** 24                    # (the 2^20 x 8 map: 1024 rows per block of squares near 10^4)
    with pytest.raises(AssertionError, match="2\\^24"):
        B.assert_partials_exact(torch.full((2047, 8), 100.0))      # 2047 rows in one block: 2.05e7
    with pytest.raises(AssertionError, match="integer"):
        B.assert_partials_exact(torch.full((4, 8), 0.5))
    for parts in (1, 129, 300, 8200):
        partial, rows, mean64, var64 = B.integer_partials(parts, 264, B.gen(parts))
        assert float(partial[:parts].max()) < 2 ** 24 and bool((var64 > 0).all()) and rows == 4 * parts


def test_a_fp32_finalize_loses_the_mean_100_columns_and_the_margin_of_the_rule_sees_it():
    """what the integer map is for: the one-pass variance from totals rounded to fp32 is off by far more than the rule
    allows in the mean-100 columns, and exact in double"""
    x = B.integer_map(1 << 20, 8, torch.bfloat16, B.gen(11)).double()
    mean64, var64 = x.mean(0), x.var(0, unbiased=False)
    s0, s1 = x.sum(0).float(), (x * x).sum(0).float()                # the totals, rounded to fp32
    inv = torch.tensor(1.0 / (1 << 20), dtype=torch.float32)
    mu = s0 * inv
    var = (s1 * inv - mu * mu).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + B.EPS)
    with pytest.raises(AssertionError, match="^invstd "):
        B.check_exact_stats(mean64.float(), invstd, mean64, var64, "fp32 finalize")
    B.check_exact_stats(mean64.float(), (1.0 / torch.sqrt(var64 + B.EPS)).float(), mean64, var64, "double finalize")


def test_feature_maps_have_no_constant_column_unless_meant():
    from tests import test_gpu_batchnorm as T
    for C in T.WIDTHS + T.SCALAR_WIDTHS:
        for rows in T.row_counts(C):
            for dtype in R.DTYPES.values():
                assert B.has_constant_column(B.feature_map(rows, C, dtype, B.gen(rows + C))) == (rows == 1)


def test_no_element_of_a_mask_recompute_case_is_inside_the_margin():
    """every call of the GPU file that recomputes the ReLU mask from z: both fp32 orders of the pre-activation give the
    float64 sign, and |a| clears MASK_MARGIN_ULPS ulps -- with zero excluded elements"""
    from tests import test_gpu_batchnorm as T
    n = elements = 0
    for tag, z, mean, invstd, gamma, beta in T.mask_recompute_cases():
        assert B.inside_mask_margin(z, mean, invstd, gamma, beta) == 0, tag
        n += 1
        elements += z.numel()
    print(f"{n} mask-recompute cases, {elements} elements, none inside the margin")
    assert n >= 3 * (len(T.WIDTHS) * 3 + 6 + 14 + 10)
    # the margin is not vacuous: an ordinary map has elements inside it before it is cleared, and none afterwards
    g = B.gen(12)
    x = B.feature_map(5003, 64, torch.bfloat16, g)
    gamma, beta = B.bn_params(64, g)
    mean, invstd = B.stats32(x)
    beta = ((mean - 1.0) * invstd * gamma).float()               # z = 1 is the zero of a
    x[::7, ::3] = 1.0
    assert B.inside_mask_margin(x, mean, invstd, gamma, beta) > 0
    assert B.inside_mask_margin(B.clear_mask_margin(x, mean, invstd, gamma, beta), mean, invstd, gamma, beta) == 0


# ---------------------------------------------------------------- the mirrors against conv.hip
WANT = {"WORKGROUPS": 1024, "PASSES": 4, "THREADS": 256, "VC": (32, 8), "VC_DIRECT": 32, "FOLD_ABOVE": 256, "FOLDS": 64,
        "CL8_MAX_C": 256, "CL_WIDE": 32, "ROW_UNROLL": 4, "VC_LOG2": (3, 5, 16), "FOLD_UNROLL": (96, 128),
        "TIERS": (15, 7, 3)}


def test_the_mirrors_restate_conv_hip():
    got = B.conv_hip_constants()
    assert got == WANT
    assert (B.WORKGROUPS, B.PASSES, B.THREADS, (B.VC_MAX, B.VC_MIN), B.FOLD_ABOVE, B.FOLDS, B.CL8_MAX_C, B.ROW_UNROLL) == \
        (got["WORKGROUPS"], got["PASSES"], got["THREADS"], got["VC"], got["FOLD_ABOVE"], got["FOLDS"], got["CL8_MAX_C"], got["ROW_UNROLL"])
    # what the shape tables of the GPU file say about themselves
    assert [B.bn_vc(C) for C in (8, 16, 64, 144, 264, 296, 512, 45)] == [1, 2, 8, 18, 11, 32, 32, 8]
    assert B.bn_parts(5003, 64) == (39, 129) and 5003 - 38 * 129 == 101
    assert B.bn_parts(1 << 20, 8) == (1024, 1024) and B.bn_parts(16384, 512) == (512, 32)
    assert B.finalize_tiers(1024, 8) == [8] and B.finalize_tiers(512, 32) == [16]
    assert B.finalize_tiers(546, 8) == [4, 1] and B.finalize_tiers(281, 32)[0] == 8          # the older tests' shapes
    assert B.finalize_tiers(97, 32)[0] == 4 and B.finalize_tiers(96, 32) == [1, 1, 1]
    assert B.finalize_tiers(225, 32)[0] == 8 and B.finalize_tiers(224, 32)[0] == 4
    assert B.finalize_tiers(1921, 8)[0] == 16 and 16 not in B.finalize_tiers(1920, 8)
    assert [B.fold_plan(p) for p in (257, 300, 6143, 6145, 8200)] == [(5, 52, False), (5, 60, False), (96, 64, False),
                                                                      (97, 64, True), (129, 64, True)]


def test_a_change_to_conv_hip_moves_the_constants():
    text = B.conv_hip_text()
    for old, new, key in (("int64_t parts = 1024 / gx;", "int64_t parts = 2048 / gx;", "WORKGROUPS"),
                          ("rows / (4 * nrl)", "rows / (8 * nrl)", "PASSES"),
                          ("for (int v = 32; v >= 8; --v)", "for (int v = 32; v >= 4; --v)", "VC"),
                          ("const int folds = 64;", "const int folds = 32;", "FOLDS"),
                          ("if (parts > 256) {", "if (parts > 512) {", "FOLD_ABOVE"),
                          ("constexpr int kBnU = 4;", "constexpr int kBnU = 8;", "ROW_UNROLL")):
        assert text.count(old) == 1, old
        assert B.conv_hip_constants(text.replace(old, new))[key] != WANT[key]
    old = "  if (C <= 256)\n    hipLaunchKernelGGL((bn_finalize_kernel<MODE, 8>)"
    assert text.count(old) == 1
    assert B.conv_hip_constants(text.replace(old, old.replace("256", "128")))["CL8_MAX_C"] == 128


# ---------------------------------------------------------------- the judge has teeth
def _bwd_outputs(rows, C, seed, relu=True, training=True):
    g = B.gen(seed)
    x = B.feature_map(rows, C, torch.float32, g)
    dy = B.randn((rows, C), torch.float32, g)
    gamma, beta = B.bn_params(C, g)
    mean, invstd = B.stats32(x)
    y = R.ref64(B.bn_fwd, x, mean, invstd, gamma, beta, None, relu=relu).float()
    on = (y > 0).double() if relu else None
    out = [t.float() for t in R.ref64(B.bn_bwd, dy, x, on, mean, invstd, gamma, training=training)]
    return out, (dy, x, on, mean, invstd, gamma)


@pytest.mark.parametrize("rows,C", [(5003, 64), (70001, 8)])
def test_a_column_sum_without_its_last_row_is_rejected(rows, C):
    (dx, dz, dg, db), ops_ = _bwd_outputs(rows, C, 20 + C)
    B.check_bwd(dx, dz, dg, db, *ops_, True, "unperturbed")
    dy, x, on, mean, invstd, gamma = ops_
    last_dz = dy[-1].double() * on[-1]
    last_xh = (x[-1].double() - mean.double()) * invstd.double()
    for c in range(C):
        if abs(float(last_dz[c])) < 0.05 or abs(float(last_xh[c])) < 0.05:
            continue                                    # (a row whose summand is next to nothing is not a row left out)
        short = db.clone()
        short[c] = float(db[c].double() - last_dz[c])
        with pytest.raises(AssertionError, match="^dbeta "):
            B.check_bwd(None, None, dg, short, *ops_, True, f"column {c} without its last row")
        short = dg.clone()
        short[c] = float(dg[c].double() - last_dz[c] * last_xh[c])
        with pytest.raises(AssertionError, match="^dgamma "):
            B.check_bwd(None, None, short, db, *ops_, True, f"column {c} without its last row")
    # and the mean of the statistics pass
    m64, _, i64 = R.ref64(B.bn_stats, x)
    B.check_stats(m64.float(), i64.float(), x, "unperturbed")
    c = int(x[-1].abs().argmax())
    short = m64.clone()
    short[c] -= x[-1, c].double() / rows
    with pytest.raises(AssertionError, match="^mean "):
        B.check_stats(short.float(), i64.float(), x, "mean without the last row")


def test_a_partial_row_counted_twice_is_rejected():
    for parts in (129, 300):
        partial, rows, mean64, var64 = B.integer_partials(parts, 8, B.gen(parts))
        p = partial[:parts].double()
        for twice in (0, parts - 1):
            s0, s1 = p[:, 0].sum(0) + p[twice, 0], p[:, 1].sum(0) + p[twice, 1]
            mean = s0 / rows
            invstd = 1.0 / torch.sqrt(s1 / rows - mean * mean + B.EPS)
            with pytest.raises(AssertionError, match="^mean "):
                B.check_exact_stats(mean.float(), invstd.float(), mean64, var64, f"partial row {twice} twice")
    (dx, dz, dg, db), ops_ = _bwd_outputs(5003, 64, 21)
    dy, x, on, mean, invstd, gamma = ops_
    block = slice(38 * 129, 5003)                       # the short last block of bn_parts(5003, 64)
    twice = db.double() + (dy.double() * on)[block].sum(0)
    with pytest.raises(AssertionError, match="^dbeta "):
        B.check_bwd(None, None, dg, twice.float(), *ops_, True, "the last partial row twice")


def test_running_statistics_faults_are_rejected():
    rows, C, c_valid = 37, 16, 13
    g = B.gen(22)
    x = B.feature_map(rows, C, torch.float32, g)
    rm0, rv0 = torch.randn(C, generator=g) * 2.0 + 1.0, torch.rand(C, generator=g) * 3.0 + 0.5
    for momentum in (0.1, 1.0):
        mean, invstd, rm, rv = (t.float() for t in R.ref64(B.stats_with_running, x, rm0, rv0, momentum=momentum, c_valid=c_valid))
        B.check_running(rm, rv, x, rm0, rv0, momentum, c_valid, "unperturbed")
        var = x.double().var(0, unbiased=False)
        biased = rv.clone()
        biased[:c_valid] = ((1 - momentum) * rv0.double() + momentum * var)[:c_valid].float()     # no rows / (rows - 1)
        with pytest.raises(AssertionError, match="^running_var "):
            B.check_running(rm, biased, x, rm0, rv0, momentum, c_valid, "no unbias factor")
        _, _, rm_all, rv_all = (t.float() for t in R.ref64(B.stats_with_running, x, rm0, rv0, momentum=momentum))
        with pytest.raises(AssertionError, match="beyond c_valid"):
            B.check_running(rm_all, rv, x, rm0, rv0, momentum, c_valid, "written beyond c_valid")
        with pytest.raises(AssertionError, match="beyond c_valid"):
            B.check_running(rm, rv_all, x, rm0, rv0, momentum, c_valid, "written beyond c_valid")


def test_a_mask_bit_from_the_unrounded_value_is_rejected():
    """fp16: a pre-activation of 1.5e-8 is positive and rounds to zero (half the smallest subnormal is 3e-8); the bit
    belongs to the stored zero"""
    C = 8
    x = torch.full((3, C), 2.0 ** -24, dtype=torch.float16)          # the smallest fp16 subnormal
    x[1] = 1.0
    mean, invstd, beta = torch.zeros(C), torch.ones(C), torch.zeros(C)
    gamma = torch.full((C,), 0.25)
    y64 = R.ref64(B.bn_fwd, x, mean, invstd, gamma, beta, None, relu=True)
    y = y64.to(torch.float16)
    assert bool((y64[0] > 0).all()) and bool((y[0] == 0).all())
    B.check_fwd(y, B.mask_bytes(y), x, mean, invstd, gamma, beta, None, True, "unperturbed")
    with pytest.raises(AssertionError, match="^mask bytes "):
        B.check_fwd(y, B.mask_bytes(y64), x, mean, invstd, gamma, beta, None, True, "bits of the unrounded y")


def _faulty_pool(x, N, H, W, k, stride, pad, last=False, transposed=False):
    """the forward with the LAST maximal tap, or with the tap index written as kj * k + ki"""
    C = x.shape[1]
    x4 = x.view(N, H, W, C)
    Ho, Wo = B.out_hw(H, W, k, stride, pad)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=x.dtype)
    tap = torch.full((N, Ho, Wo, C), -1, dtype=torch.int64)
    for ki, kj, h, w, inside in B._taps(H, W, k, stride, pad):
        v = x4[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
        take = inside.view(1, Ho, Wo, 1) & ((tap < 0) | ((v >= best) if last else (v > best)))
        best = torch.where(take, v, best)
        tap = torch.where(take, torch.full_like(tap, kj * k + ki if transposed else ki * k + kj), tap)
    return best.reshape(-1, C), tap.to(torch.uint8).reshape(-1, C)


@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (2, 2, 0), (5, 2, 2)])
def test_pool_forward_faults_are_rejected(k, stride, pad):
    N, C, H, W = 3, 16, 9, 11
    geom = dict(N=N, H=H, W=W, k=k, stride=stride, pad=pad)
    x = ((torch.randn(N * H * W, C, generator=B.gen(23), dtype=D64).clamp_min(0) * 4).round() / 4).to(torch.bfloat16)
    y, tap = B.maxpool_fwd(x, **geom)
    B.check_maxpool_fwd(y, tap, x, geom, "unperturbed")
    for fault in ({"last": True}, {"transposed": True}):
        fy, ftap = _faulty_pool(x, **geom, **fault)
        assert torch.equal(fy, y)                       # (the values are those of a correct pool: only the taps tell)
        with pytest.raises(AssertionError, match="^tap bytes "):
            B.check_maxpool_fwd(fy, ftap, x, geom, str(fault))
    z = B.tie_map(N * H * W, C, torch.float16, B.gen(24))
    one, zero = torch.ones(C), torch.zeros(C)
    if (k, stride, pad) == (3, 2, 1):
        p, t = B.stem_fwd(z, zero, one, one, zero, N, H, W, True, torch.float16)
        B.check_stem_fwd(p, t, z, zero, one, one, zero, N, H, W, True, "unperturbed")
        with pytest.raises(AssertionError, match="^tap bytes "):
            B.check_stem_fwd(p, _faulty_pool(z, **geom, last=True)[1], z, zero, one, one, zero, N, H, W, True, "last tap")


@pytest.mark.parametrize("integer", [False, True])
def test_a_pool_backward_without_the_second_window_is_rejected(integer):
    """(3, 2, 1): a pixel with an odd coordinate lies in two windows along that axis (taps 0 and 2); the fault leaves out
    the window that holds it as tap row 2"""
    N, C, H, W = 3, 16, 9, 11
    geom = dict(N=N, H=H, W=W, k=3, stride=2, pad=1)
    g = B.gen(25)
    x = B.randn((N * H * W, C), torch.float32, g)
    _, tap = B.maxpool_fwd(x, **geom)
    dy = B.integer_grad(tap.shape[0], C, torch.float32, g) if integer else B.randn(tuple(tap.shape), torch.float32, g)
    dx = B.maxpool_bwd(dy.double(), tap, **geom).float()
    B.check_maxpool_bwd(dx, dy, tap, geom, "unperturbed", exact=integer)
    kept = torch.where(tap // 3 == 2, torch.zeros_like(dy), dy)
    faulty = B.maxpool_bwd(kept.double(), tap, **geom).float()
    assert not torch.equal(faulty, dx)
    with pytest.raises(AssertionError, match="^dx "):
        B.check_maxpool_bwd(faulty, dy, tap, geom, "second window left out", exact=integer)


def test_an_eval_backward_with_the_train_correction_is_rejected():
    (dx_train, dz, dg, db), ops_ = _bwd_outputs(37, 16, 26, training=True)
    (dx_eval, _, _, _), _ = _bwd_outputs(37, 16, 26, training=False)
    B.check_bwd(dx_eval, dz, dg, db, *ops_, False, "unperturbed")
    B.check_bwd(dx_train, dz, dg, db, *ops_, True, "unperturbed")
    with pytest.raises(AssertionError, match="^dx "):
        B.check_bwd(dx_train, None, None, None, *ops_, False, "train correction left in")
    with pytest.raises(AssertionError, match="^dx "):
        B.check_bwd(dx_eval, None, None, None, *ops_, True, "train correction left out")


def test_the_fp32_chain_is_inside_the_rule_on_the_chosen_inputs():
    """what the rule asks of a kernel, asked of the plain fp32 evaluation rounded once to the output type"""
    from tests import test_gpu_batchnorm as T
    for name, dtype in R.DTYPES.items():
        for rows, C in ((5, 8), (T.SHORT_LAST[0], T.SHORT_LAST[1]), (37, 264), (300, 45)):
            x, res, gamma, beta, mean, invstd = T._fwd_case(rows, C, dtype, rows + C)
            for m, _, i in (R.fp32_chain(B.bn_stats, x), B.bn_stats_chain(x)):     # the two-pass and the one-pass chain
                B.check_stats(m, i, x, f"{name} {rows}x{C}")
            for relu in (True, False):
                y = R.fp32_chain(B.bn_fwd, x, mean, invstd, gamma, beta, res, relu=relu).to(dtype)
                B.check_fwd(y, B.mask_bytes(y) if C % 8 == 0 else None, x, mean, invstd, gamma, beta, res, relu, f"{name} {rows}x{C}")
            for src in ("z", "y", "mask") if C % 8 == 0 else ("z", "y"):
                dy, xc, y, mask, on, *_ = T._bwd_case(rows, C, dtype, rows + C, src, True)
                for training in (True, False):
                    dx, dz, dg, db = R.fp32_chain(B.bn_bwd, dy, xc, on, mean, invstd, gamma, training=training)
                    B.check_bwd(dx.to(dtype), dz.to(dtype), dg, db, dy, xc, on, mean, invstd, gamma, training, f"{name} {src} {rows}x{C}")
