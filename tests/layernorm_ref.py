"""Plain torch-CPU statements of the LayerNorm kernels (csrc/layernorm.hip, csrc/ln_reduce.h) and of the cross-entropy on
integer labels (csrc/losses.hip), the operand magnitudes their outputs are judged by, and the input builders of
tests/test_gpu_layernorm.py.  No GPU is touched here; tests/test_layernorm_cpu.py checks this file.

Every operation works in whatever floating dtype it is handed, for ``ref64`` / ``fp32_chain`` of tests/rowwise_ref.py.
Rows are the first axis: x, y, dy, dx are [rows, d]; gamma, beta, dgamma, dbeta are [d]; mean, rstd are [rows]."""
from __future__ import annotations

import math

import torch

from tests import rowwise_ref as R

EPS = float(torch.tensor(1e-5, dtype=torch.float32))     # the kernel takes eps as a float: both sides see that value


# ---------------------------------------------------------------- LayerNorm
def ln_fwd(x, gamma, beta, eps=EPS):
    """two passes, as the kernel states it: the mean, then the variance of the centred values -> (y, mean, rstd)"""
    mean = x.mean(1)
    xc = x - mean.unsqueeze(1)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1) + eps)
    return xc * rstd.unsqueeze(1) * gamma + beta, mean, rstd


def _first_rows(t, n1):
    """[rows, d] -> the view [n0, d] of rows (i0, 0)"""
    return t.view(t.shape[0] // n1, n1, t.shape[1])[:, 0]


def ln_bwd_terms(dy, x, gamma, mean, rstd, dy_first=None, n1=1):
    """-> (dy with dy_first added to rows (i0, 0), xhat, g = dy gamma, mean(g), mean(g xhat)) from the statistics handed in"""
    if dy_first is not None:
        dy = dy.clone()
        _first_rows(dy, n1).add_(dy_first)
    xh = (x - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    g = dy * gamma
    return dy, xh, g, g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)


def ln_bwd(dy, x, gamma, mean, rstd, dx_add=None, dy_first=None, dx_first=None, n1=1):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, from the ``mean`` / ``rstd`` the backward kernel is handed
    (not recomputed: the backward is judged independently of the forward); dgamma = sum_rows dy xhat, dbeta = sum_rows dy.
    ``dy_first`` [n0, d] is added to dy of row (i0, 0) before anything else, so it enters dgamma and dbeta as well;
    ``dx_first`` [n0, d] and ``dx_add`` [rows, d] are added to dx only.  -> (dx, dgamma, dbeta)"""
    dy, xh, g, c1, c2 = ln_bwd_terms(dy, x, gamma, mean, rstd, dy_first, n1)
    dx = rstd.unsqueeze(1) * (g - c1 - xh * c2)
    if dx_add is not None:
        dx = dx + dx_add
    if dx_first is not None:
        dx = dx.clone()
        _first_rows(dx, n1).add_(dx_first)
    return dx, (dy * xh).sum(0), dy.sum(0)


# ---------------------------------------------------------------- what lies behind each output element (float64)
def y_mag(x, gamma, beta, eps=EPS):
    """max(|xhat gamma|, |beta|, rstd |gamma| max(|x|, |mean|)) per element of y.  The last term is what the first two
    leave out: xhat_i = rstd (x_i - mean) is a difference of two operands of magnitude |x_i| and |mean|, and the fp32
    mean's own rounding (half an ulp of |mean|, whatever the order of summation) reaches y_i as an absolute error of
    rstd |gamma_i| ulp(mean) / 2 -- where xhat_i is near zero that is many ulps of |xhat_i gamma_i|.  With the first two
    terms alone a second fp32 evaluation of ln_fwd that only sums in another order falls outside the rule at such
    elements (3 of 200 shapes of this file's inputs), so no correct kernel could be expected inside it."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    y, mean, rstd = ln_fwd(x, gamma, beta, eps)
    m = torch.maximum((y - beta).abs(), beta.abs().expand_as(y))
    return torch.maximum(m, rstd.unsqueeze(1) * gamma.abs() * torch.maximum(x.abs(), mean.abs().unsqueeze(1)))


def bwd_mags(dy, x, gamma, mean, rstd, dx_add=None, dy_first=None, dx_first=None, n1=1):
    """-> (dx_mag [rows, d], dgamma_mag [d], dbeta_mag [d]): rstd max(|g|, |mean(g)|, |xhat mean(g xhat)|) with the added
    operands; the largest summand of each dgamma / dbeta column"""
    args = [None if t is None else t.double() for t in (dy, x, gamma, mean, rstd, dy_first)]
    dy, xh, g, c1, c2 = ln_bwd_terms(*args, n1=n1)
    m = rstd.double().unsqueeze(1) * torch.maximum(torch.maximum(g.abs(), c1.abs().expand_as(g)), (xh * c2).abs())
    if dx_add is not None:
        m = torch.maximum(m, dx_add.double().abs())
    if dx_first is not None:
        m = m.clone()
        f = _first_rows(m, n1)
        f.copy_(torch.maximum(f, dx_first.double().abs()))
    return m, (dy * xh).abs().max(0).values, dy.abs().max(0).values


# ---------------------------------------------------------------- judging a kernel's outputs (CPU tensors)
def stats32(x, gamma, beta, eps=EPS):
    """the mean / rstd the backward is handed: the float64 reference's, rounded to fp32"""
    _, mean, rstd = R.ref64(ln_fwd, x, gamma, beta, eps=eps)
    return mean.float(), rstd.float()


def check_fwd(y, mean, rstd, x, gamma, beta, tag, eps=EPS):
    """y [rows, d] in its own dtype, mean / rstd [rows] f32 against ln_fwd of the (rounded) operands"""
    ref = R.ref64(ln_fwd, x, gamma, beta, eps=eps)
    chain = R.fp32_chain(ln_fwd, x, gamma, beta, eps=eps)
    R.assert_close(y, ref[0], chain[0], y_mag(x, gamma, beta, eps), f"y {tag}")
    R.assert_close(mean, ref[1], chain[1], x.double().abs().max(1).values, f"mean {tag}")     # a sum of x_j / d
    R.assert_close(rstd, ref[2], chain[2], 0.0, f"rstd {tag}")                                # (its own magnitude)


def check_bwd(dx, dg, db, dy, x, gamma, mean, rstd, tag, *, dx_add=None, dy_first=None, dx_first=None, n1=1, dg0=None,
              db0=None, dx_lp=None):
    """dx [rows, d] (and its 16-bit copy ``dx_lp``), dgamma / dbeta [d] against ln_bwd; ``dg0`` / ``db0``: what dgamma /
    dbeta held before an accumulating call.  An output given as None is not judged."""
    ops = (dy, x, gamma, mean, rstd, dx_add, dy_first, dx_first)
    ref = R.ref64(ln_bwd, *ops, n1=n1)
    chain = R.fp32_chain(ln_bwd, *ops, n1=n1)
    m_dx, m_dg, m_db = bwd_mags(dy, x, gamma, mean, rstd, dx_add, dy_first, dx_first, n1)
    if dx is not None:
        R.assert_close(dx, ref[0], chain[0], m_dx, f"dx {tag}")
    if dx_lp is not None:
        assert dx_lp.dtype in (torch.bfloat16, torch.float16)
        R.assert_close(dx_lp, ref[0], chain[0], m_dx, f"dx_lp {tag}")
    for got, r, c, m, base, what in ((dg, ref[1], chain[1], m_dg, dg0, "dgamma"), (db, ref[2], chain[2], m_db, db0, "dbeta")):
        if got is None:
            continue
        if base is not None:                             # one more summand
            r, c, m = r + base.double(), c + base.float(), torch.maximum(m, base.double().abs())
        R.assert_close(got, r, c, m, f"{what} {tag}")


# ---------------------------------------------------------------- cross-entropy on integer labels
def ce_labels(logits, labels, ignore_index=-100):
    """nn.CrossEntropyLoss()(logits, labels): the mean of lse - logit[label] over the rows whose label is not
    ``ignore_index`` -> (loss [], lse [M], count []).  No counted row: 0 / 0 = NaN.  A label outside [0, C) that is not
    ignore_index makes the loss NaN (the kernel's statement; torch raises)."""
    M, C = logits.shape
    lse = torch.logsumexp(logits, 1)
    keep = labels != ignore_index
    bad = keep & ((labels < 0) | (labels >= C))
    nll = lse - logits.gather(1, labels.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    nll = torch.where(bad, torch.full_like(nll, math.nan), nll)
    count = keep.sum().to(logits.dtype)
    return torch.where(keep, nll, torch.zeros_like(nll)).sum() / count, lse, count


def ce_labels_bwd(logits, labels, lse, count, gloss, ignore_index=-100):
    """dlogits = gloss / count (softmax - onehot) from the ``lse`` and ``count`` the backward kernel is handed; an ignored
    row is exactly zero whatever gloss / count is, a row with an out-of-range label is NaN"""
    M, C = logits.shape
    keep = (labels != ignore_index).unsqueeze(1)
    bad = keep & ((labels < 0) | (labels >= C)).unsqueeze(1)
    onehot = torch.arange(C).unsqueeze(0) == labels.unsqueeze(1)
    d = gloss.reshape(()) / count.reshape(()) * (torch.exp(logits - lse.unsqueeze(1)) - onehot.to(logits.dtype))
    d = torch.where(bad, torch.full_like(d, math.nan), d)
    return torch.where(keep, d, torch.zeros_like(d))


# ---------------------------------------------------------------- input builders
def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, dtype, g, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift).to(dtype)


def ln_params(d, g):
    """gamma, beta f32 [d]: gamma around 1 with both signs of deviation, never near 0"""
    gamma = (1.0 + 0.25 * torch.randn(d, generator=g, dtype=torch.float64).clamp(-3, 3)).float()
    beta = (0.3 * torch.randn(d, generator=g, dtype=torch.float64)).float()
    return gamma, beta


def offset_rows(rows, d, dtype, g, mean=100.0):
    """rows whose mean is far from zero against a small spread (0.1): a one-pass variance E[x^2] - E[x]^2 loses its digits
    in fp32 (1e4 against 1e-2), the two-pass one does not.  fp16 holds steps of 1/16 at 100 and the values fall on them.
    bf16 holds steps of 1/2 only: there the spread is 0.75, so that a row is more than one value (and such values and
    their squares are exact in fp32, so in bf16 the rows test the large mean, not the one-pass loss).  Columns 0 and 1
    are set one step apart, so that no row is constant after rounding."""
    spread, step = {torch.float32: (0.1, 0.1), torch.bfloat16: (0.75, 0.5), torch.float16: (0.1, 0.0625)}[dtype]
    x = (mean + spread * torch.randn(rows, d, generator=g, dtype=torch.float64)).to(dtype)
    x[:, 0] = mean
    x[:, 1] = mean + step
    return x


def constant_rows(rows, d, dtype, value=3.0):
    """every element equal: the variance is exactly zero and rstd = 1 / sqrt(eps)"""
    return torch.full((rows, d), value, dtype=torch.float64).to(dtype)


def fp16_top_rows(rows, d, g):
    """fp16 elements of both signs between 3e4 and 6e4 (fp16's largest finite value is 65504)"""
    mag = 3.0e4 + 3.0e4 * torch.rand(rows, d, generator=g, dtype=torch.float64)
    sgn = torch.where(torch.rand(rows, d, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sgn).to(torch.float16)


def ce_case(M, C, dtype, g, ignore_index=-100, ignored="wave"):
    """(logits [M, C] in ``dtype``, labels [M] int64).  ``ignored``: "wave" -- rows 1, 17, 33, ... (all the rows of wave 1
    of sixteen) and row 2 are ignored (with M = 1 nothing is); "all" -- every row; "none"."""
    logits = randn((M, C), dtype, g, 3.0)
    labels = torch.randint(0, C, (M,), generator=g)
    if M > 1:
        labels[0], labels[M - 1] = C - 1, 0                 # the two ends of the class range
    if ignored == "all":
        labels[:] = ignore_index
    elif ignored == "wave":
        labels[1::16] = ignore_index
        if M > 3:
            labels[2] = ignore_index
    return logits, labels
