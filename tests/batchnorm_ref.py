"""Plain torch-CPU statements of the BatchNorm and max-pool kernels of csrc/conv.hip, the operand magnitudes their outputs
are judged by, Python mirrors of the host-side partition (bn_vc, bn_vc_log2, bn_parts, the finalize kernel's column lanes
and loop tiers) and the input builders of tests/test_gpu_batchnorm.py.  No GPU is touched here;
tests/test_batchnorm_cpu.py checks this file.

Every operation works in whatever floating dtype it is handed, for ``ref64`` / ``fp32_chain`` of tests/rowwise_ref.py, and is
written from the operation's definition, not from the kernel.  Maps are NHWC rows: x, y, dy, dx are [rows, C] (rows =
N H W for the pooling operations); mean, invstd, gamma, beta, dgamma, dbeta are [C].

Column sums over many rows (mean, variance, dgamma, dbeta) go through ``colsum``.  In fp32 it is the plain sequential
sum r = 0, 1, 2, ... of the rows, every addition rounded to fp32: the least favourable order a correct kernel may use
(its error grows with the row count, where a pairwise or lane-strided order grows with its logarithm or its square root).
The kernels' orders -- lane-strided fp32 sums over at most rows_per_block rows, a fixed lane order, then double precision
across the partial rows -- lie inside it, so four times this chain's own error is a bound no correct kernel exceeds and one
that a dropped or doubled row of a column does (tests/test_batchnorm_cpu.py shows the second half).  torch's own cumsum
and sum accumulate fp32 columns in double on the CPU, which is why numpy's float32 cumsum states the chain."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch

from tests import rowwise_ref as R

EPS = float(torch.tensor(1e-5, dtype=torch.float32))     # the kernels take eps as a float: both sides see that value


def gen(seed):
    return torch.Generator().manual_seed(seed)


def colsum(t):
    """[rows, ...] -> the sum over the rows: sequential fp32 additions for an fp32 tensor, torch's sum otherwise"""
    if t.dtype == torch.float32:
        a = np.ascontiguousarray(t.detach().numpy())
        return torch.from_numpy(np.cumsum(a, axis=0, dtype=np.float32)[-1].copy())
    return t.sum(0)


# ---------------------------------------------------------------- statistics
def bn_stats(x, eps=EPS):
    """two passes: the mean, then the (biased) variance of the centred values -> (mean, var, invstd)"""
    rows = x.shape[0]
    mean = colsum(x) / rows
    xc = x - mean
    var = colsum(xc * xc) / rows
    return mean, var, 1.0 / torch.sqrt(var + eps)


def running_update(run_mean, run_var, mean, var, rows, momentum, c_valid=None):
    """nn.BatchNorm's update from the batch mean and the biased batch variance: the variance enters unbiased, rows /
    (rows - 1), and as it is at rows == 1; only the first ``c_valid`` channels are touched -> (run_mean, run_var)"""
    cv = run_mean.shape[0] if c_valid is None else c_valid
    unbias = rows / (rows - 1) if rows > 1 else 1.0
    rm, rv = run_mean.clone(), run_var.clone()
    rm[:cv] = (1.0 - momentum) * run_mean[:cv] + momentum * mean[:cv]
    rv[:cv] = (1.0 - momentum) * run_var[:cv] + momentum * (var[:cv] * unbias)
    return rm, rv


def stats_with_running(x, run_mean, run_var, momentum=0.1, eps=EPS, c_valid=None):
    mean, var, invstd = bn_stats(x, eps)
    rm, rv = running_update(run_mean, run_var, mean, var, x.shape[0], momentum, c_valid)
    return mean, invstd, rm, rv


def stats_from_partials(partial, rows, eps=EPS):
    """partial [parts, 2, C] = (sum x, sum x^2) over disjoint sets of rows -> (mean, var, invstd)"""
    mean = colsum(partial[:, 0]) / rows
    var = (colsum(partial[:, 1]) / rows - mean * mean).clamp_min(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def rsqrt_eps(var, eps=EPS):
    return 1.0 / torch.sqrt(var + eps)


# ---------------------------------------------------------------- forward
def padded(p, C):
    """gamma / beta of a channel-padded layer: the channels beyond the c_valid real ones are exact zeros"""
    return p if p.shape[0] == C else torch.cat([p, torch.zeros(C - p.shape[0], dtype=p.dtype)])


def affine(x, mean, invstd, gamma, beta):
    C = x.shape[1]
    return (x - mean) * invstd * padded(gamma, C) + padded(beta, C)


def bn_fwd(x, mean, invstd, gamma, beta, residual=None, relu=False):
    """relu?(xhat gamma + beta (+ residual)), before the rounding to the map's dtype"""
    y = affine(x, mean, invstd, gamma, beta)
    if residual is not None:
        y = y + residual
    return y.clamp_min(0) if relu else y


def mask_bytes(y):
    """bit k of byte (r, g) is y[r, 8 g + k] > 0, on the y that was stored (rounded to its dtype)"""
    rows, C = y.shape
    bits = (y.float() > 0).view(rows, C // 8, 8).to(torch.int32)
    return (bits << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def mask_bits(mask, C):
    """mask bytes [rows, C / 8] -> 0 / 1 [rows, C] (float64)"""
    b = (mask.to(torch.int32).unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1
    return b.reshape(mask.shape[0], C).double()


def fwd_mag(x, mean, invstd, gamma, beta, residual=None):
    """max(|xhat gamma|, |beta|, invstd |gamma| max(|x|, |mean|), |residual|) per element of y: the third term is the
    rounding of the difference x - mean as seen from y (layernorm_ref.y_mag gives the arithmetic)"""
    x, mean, invstd = x.double(), mean.double(), invstd.double()
    g, b = padded(gamma.double(), x.shape[1]), padded(beta.double(), x.shape[1])
    m = torch.maximum(((x - mean) * invstd * g).abs(), b.abs().expand_as(x))
    m = torch.maximum(m, invstd * g.abs() * torch.maximum(x.abs(), mean.abs().expand_as(x)))
    return m if residual is None else torch.maximum(m, residual.double().abs())


# ---------------------------------------------------------------- backward
def bn_bwd(dy, x, on, mean, invstd, gamma, training=True):
    """dz = dy * on (``on``: 0 / 1 per element from the source the call uses, None without a ReLU);
    train: dx = gamma invstd (dz - sum(dz) / rows - xhat sum(dz xhat) / rows), eval: dx = gamma invstd dz; dres = dz;
    -> (dx, dz, dgamma, dbeta) from the ``mean`` / ``invstd`` the kernel is handed"""
    rows, C = x.shape
    g = padded(gamma, C)
    dz = dy if on is None else dy * on
    xh = (x - mean) * invstd
    dgamma, dbeta = colsum(dz * xh), colsum(dz)
    if training:
        dx = g * invstd * (dz - dbeta / rows - xh * (dgamma / rows))
    else:
        dx = g * invstd * dz
    return dx, dz, dgamma, dbeta


def bwd_mags(dy, x, on, mean, invstd, gamma, training=True, dy_mag=None):
    """-> (dx_mag [rows, C], dgamma_mag [C], dbeta_mag [C]).  dgamma = sum_r dz xhat and dbeta = sum_r dz run over up to
    millions of rows, and an fp32 addition rounds at the magnitude of its result, a partial sum.  Which partial sums are
    formed depends on the order (rows of one lane, lanes of one workgroup, ...), but none of any order exceeds the sum of
    the summands' magnitudes: dgamma_mag = sum |dz xhat|, dbeta_mag = sum |dz|.  (The largest summand, which serves
    layernorm_ref's columns of a few rows, is below the partial sums a correct kernel forms here: with 16-bit data or few
    columns the sequential chain can come out exact and leave one ulp of a single summand for a sum of 150 of them.)
    The same holds for the two means in dx: dx_mag = |gamma| invstd max(|dz|, mean |dz|, |xhat| mean |dz xhat|).
    ``dy_mag``: where dy is itself a sum (the gradient gathered from up to four pooling windows), the sum of the magnitudes
    of what was gathered, in place of |dy|."""
    dy, x, mean, invstd = dy.double(), x.double(), mean.double(), invstd.double()
    rows, C = x.shape
    g = padded(gamma.double(), C)
    dzm = dy.abs() if dy_mag is None else dy_mag.double()
    dzm = dzm if on is None else dzm * on.double()
    xh = ((x - mean) * invstd).abs()
    m = dzm
    if training:
        m = torch.maximum(m, (dzm.sum(0) / rows).expand_as(m))
        m = torch.maximum(m, xh * ((dzm * xh).sum(0) / rows))
    return (g * invstd).abs() * m, (dzm * xh).sum(0), dzm.sum(0)


# ---------------------------------------------------------------- max-pool (NHWC rows)
def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _taps(H, W, k, stride, pad):
    """(ki, kj, h [Ho], w [Wo], inside [Ho, Wo]) per tap in scan order"""
    Ho, Wo = out_hw(H, W, k, stride, pad)
    for ki in range(k):
        for kj in range(k):
            h = torch.arange(Ho) * stride - pad + ki
            w = torch.arange(Wo) * stride - pad + kj
            yield ki, kj, h, w, ((h >= 0) & (h < H)).unsqueeze(1) & ((w >= 0) & (w < W)).unsqueeze(0)


def maxpool_fwd(x, N, H, W, k, stride, pad):
    """x [N H W, C] -> (y [N Ho Wo, C], tap uint8 [N Ho Wo, C]): the value and the index ki * k + kj of the FIRST maximum in
    scan order over the taps that lie inside the image"""
    C = x.shape[1]
    x4 = x.view(N, H, W, C)
    Ho, Wo = out_hw(H, W, k, stride, pad)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=x.dtype)
    tap = torch.full((N, Ho, Wo, C), -1, dtype=torch.int64)
    for ki, kj, h, w, inside in _taps(H, W, k, stride, pad):
        v = x4[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
        take = inside.view(1, Ho, Wo, 1) & ((tap < 0) | (v > best))
        best = torch.where(take, v, best)
        tap = torch.where(take, torch.full_like(tap, ki * k + kj), tap)
    assert bool((tap >= 0).all()), "a window without a tap inside the image"
    return best.reshape(-1, C), tap.to(torch.uint8).reshape(-1, C)


def maxpool_bwd(dy, tap, N, H, W, k, stride, pad):
    """dy, tap [N Ho Wo, C] -> dx [N H W, C]: every window's gradient goes to the pixel its tap byte names"""
    C = dy.shape[1]
    Ho, Wo = out_hw(H, W, k, stride, pad)
    dy4, tap4 = dy.view(N, Ho, Wo, C), tap.view(N, Ho, Wo, C)
    dx = torch.zeros(N, H, W, C, dtype=dy.dtype)
    for ki, kj, h, w, inside in _taps(H, W, k, stride, pad):
        sel = (tap4 == ki * k + kj) & inside.view(1, Ho, Wo, 1)
        contrib = torch.where(sel, dy4, torch.zeros_like(dy4))
        hv, wv = ((h >= 0) & (h < H)).nonzero().flatten(), ((w >= 0) & (w < W)).nonzero().flatten()
        if len(hv) and len(wv):                 # (within one tap distinct windows name distinct pixels)
            dx[:, h[hv].unsqueeze(1), w[wv].unsqueeze(0)] += contrib[:, hv.unsqueeze(1), wv.unsqueeze(0)]
    return dx.reshape(-1, C)


def maxpool_bwd_mag(dy, tap, N, H, W, k, stride, pad):
    """the largest |dy| that reaches each pixel"""
    C = dy.shape[1]
    Ho, Wo = out_hw(H, W, k, stride, pad)
    dy4, tap4 = dy.double().abs().view(N, Ho, Wo, C), tap.view(N, Ho, Wo, C)
    m = torch.zeros(N, H, W, C, dtype=torch.float64)
    for ki, kj, h, w, inside in _taps(H, W, k, stride, pad):
        sel = (tap4 == ki * k + kj) & inside.view(1, Ho, Wo, 1)
        contrib = torch.where(sel, dy4, torch.zeros_like(dy4))
        hv, wv = ((h >= 0) & (h < H)).nonzero().flatten(), ((w >= 0) & (w < W)).nonzero().flatten()
        if len(hv) and len(wv):
            cur = m[:, h[hv].unsqueeze(1), w[wv].unsqueeze(0)]
            m[:, h[hv].unsqueeze(1), w[wv].unsqueeze(0)] = torch.maximum(cur, contrib[:, hv.unsqueeze(1), wv.unsqueeze(0)])
    return m.reshape(-1, C)


# ---------------------------------------------------------------- the fused stem: BatchNorm (+ ReLU) + max-pool(3, 2, 1)
def stem_fwd(z, mean, invstd, gamma, beta, N, H, W, relu, dtype):
    """the forward rounded to the map's dtype, then the pool -> (pooled in ``dtype``, tap bytes)"""
    y = bn_fwd(z.double(), mean.double(), invstd.double(), gamma.double(), beta.double(), None, relu).to(dtype)
    return maxpool_fwd(y, N, H, W, 3, 2, 1)


def stem_bwd(dyp, z, on, mean, invstd, gamma, tap, N, H, W, training=True):
    """the BatchNorm backward on dy gathered from the pooled gradient (never rounded in between) -> bn_bwd's tuple"""
    return bn_bwd(maxpool_bwd(dyp, tap, N, H, W, 3, 2, 1), z, on, mean, invstd, gamma, training)


# ---------------------------------------------------------------- judging a kernel's outputs (CPU tensors)
def _report(what, got, ref, chain, mag):
    """worst error over budget of an fp32 output, printed before the assertion (run with -s to see it)"""
    E = R.budget(ref.double(), chain, mag)
    err = (got.double() - ref.double()).abs()
    cerr = (chain.double() - ref.double()).abs()
    i = int((err / E).argmax())
    print(f"[budget] {what}: worst |err| / E = {float((err / E).max()):.3f} (err {float(err.flatten()[i]):.3e}, E "
          f"{float(E.flatten()[i]):.3e}, chain's own worst error {float(cerr.max()):.3e})")


def stats32(x, eps=EPS):
    """the mean / invstd the forward and backward kernels are handed: the float64 reference's, rounded to fp32"""
    mean, _, invstd = R.ref64(bn_stats, x, eps=eps)
    return mean.float(), invstd.float()


def invstd_mag(x, eps=EPS):
    """invstd^3 E[x^2] / 2 per column: what one fp32 ulp of E[x^2] is worth in invstd.  The kernels read the map once, so
    the variance they form is E[x^2] - mean^2, a difference of two operands of that magnitude: the fp32 rounding of the
    squares and of their partial sums (half an ulp of E[x^2] at the least, whatever the order of summation and however
    precisely the partial rows are added up afterwards) reaches invstd = (var + eps)^(-1/2) multiplied by invstd^3 / 2.
    Against invstd's own ulp that is E[x^2] / (var + eps) times as much: nothing at mean 0, everything at rows = 1, where
    var is 0 and eps = 1e-5 stands against the rounding of x^2 itself.  The two-pass statement of this file has no such term
    (it is what the result should be), so with invstd's own magnitude alone no one-pass kernel could be inside the rule; on
    the integer maps, whose squares and sums are exact, check_exact_stats asks for invstd's own ulp."""
    x = x.double()
    _, _, invstd = bn_stats(x, eps)
    return 0.5 * invstd ** 3 * (x * x).mean(0)


def bn_stats_chain(x, eps=EPS):
    """the fp32 chain of the statistics -> (mean, var, invstd) f32.  The reference is the two-pass statement; the chain is
    the sums a one-pass kernel has to form -- sum x and sum x^2, each the sequential fp32 sum of colsum, every square
    rounded to fp32 -- put together in double (mean = s0 / rows, var = s1 / rows - mean^2: conv.hip states that its finalize
    adds the partial rows and forms the variance in double, and the integer maps hold it to that) and rounded to fp32.
    Four times this chain's error is the room the rule leaves for the order in which the kernels add the squares: a
    two-pass fp32 chain would leave room in units of the variance, where the rounding of a sum of squares comes in units of
    E[x^2] (see invstd_mag), and not even three rows could be added inside it."""
    rows = x.shape[0]
    x32 = x.float()
    mean = colsum(x32).double() / rows
    var = (colsum(x32 * x32).double() / rows - mean * mean).clamp_min(0).float()
    return mean.float(), var, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def check_stats(mean, invstd, x, tag, eps=EPS):
    ref = R.ref64(bn_stats, x, eps=eps)
    chain = bn_stats_chain(x, eps)
    R.assert_close(mean, ref[0], chain[0], x.double().abs().max(0).values, f"mean {tag}")
    R.assert_close(invstd, ref[2], chain[2], invstd_mag(x, eps), f"invstd {tag}")


def check_running(rm, rv, x, rm0, rv0, momentum, c_valid, tag, eps=EPS):
    """the running statistics after one bn_stats from ``rm0`` / ``rv0``; the channels beyond c_valid must be untouched"""
    ref = R.ref64(stats_with_running, x, rm0, rv0, momentum=momentum, eps=eps, c_valid=c_valid)
    cmean, cvar, _ = bn_stats_chain(x, eps)                                   # (the one-pass chain: see bn_stats_chain)
    chain = (None, None) + running_update(rm0.float(), rv0.float(), cmean, cvar, x.shape[0], momentum, c_valid)
    x64 = x.double()
    xc2 = (x64 * x64).mean(0) * (x.shape[0] / max(x.shape[0] - 1, 1))      # (E[x^2], unbiased: see invstd_mag)
    assert torch.equal(rm[c_valid:], rm0[c_valid:]) and torch.equal(rv[c_valid:], rv0[c_valid:]), \
        f"running statistics {tag}: a channel beyond c_valid = {c_valid} was written"
    R.assert_close(rm, ref[2], chain[2], torch.maximum(rm0.double().abs(), x64.abs().max(0).values), f"running_mean {tag}")
    R.assert_close(rv, ref[3], chain[3], torch.maximum(rv0.double().abs(), xc2), f"running_var {tag}")


def check_exact_stats(mean, invstd, mean64, var64, tag, eps=EPS):
    """inputs whose sums the kernels form exactly: the mean is the float64 mean rounded to fp32; invstd is within the rule
    of rsqrt(var64 + eps), the chain being 1 / sqrt in fp32 of the exact variance"""
    assert torch.equal(mean, mean64.float()), \
        f"mean {tag}: not the exact mean rounded to fp32 (worst {float((mean.double() - mean64).abs().max()):.3e})"
    chain = 1.0 / torch.sqrt(var64.float() + torch.tensor(eps, dtype=torch.float32))
    R.assert_close(invstd, 1.0 / torch.sqrt(var64 + eps), chain, 0.0, f"invstd {tag}")


def check_fwd(y, mask, x, mean, invstd, gamma, beta, residual, relu, tag):
    """y in its own dtype against bn_fwd; the mask bytes (if any) against the y that was stored"""
    ops_ = (x, mean, invstd, gamma, beta, residual)
    R.assert_close(y, R.ref64(bn_fwd, *ops_, relu=relu), R.fp32_chain(bn_fwd, *ops_, relu=relu),
                   fwd_mag(x, mean, invstd, gamma, beta, residual), f"y {tag}")
    if mask is not None:
        assert mask.dtype == torch.uint8 and torch.equal(mask, mask_bytes(y)), f"mask bytes {tag}: not (stored y > 0)"


def check_bwd(dx, dres, dg, db, dy, x, on, mean, invstd, gamma, training, tag, *, dg0=None, db0=None, c_valid=None,
              report=False):
    """dx / dres [rows, C] in their dtype, dgamma / dbeta [c_valid] f32 against bn_bwd; ``dg0`` / ``db0``: what dgamma / dbeta
    held before an accumulating call.  An output given as None is not judged."""
    ops_ = (dy, x, on, mean, invstd, gamma)
    ref = R.ref64(bn_bwd, *ops_, training=training)
    chain = R.fp32_chain(bn_bwd, *ops_, training=training)
    m_dx, m_dg, m_db = bwd_mags(dy, x, on, mean, invstd, gamma, training)
    cv = x.shape[1] if c_valid is None else c_valid
    if dx is not None:
        R.assert_close(dx, ref[0], chain[0], m_dx, f"dx {tag}")
    if dres is not None:                                    # dz = dy or 0: no arithmetic at all
        assert torch.equal(dres.double(), ref[1]), f"dres {tag}: not dy under the mask"
    for got, r, c, m, base, what in ((dg, ref[2], chain[2], m_dg, dg0, "dgamma"), (db, ref[3], chain[3], m_db, db0, "dbeta")):
        if got is None:
            continue
        r, c, m = r[:cv], c[:cv], m[:cv]
        if base is not None:                                # one more summand
            r, c, m = r + base.double(), c + base.float(), torch.maximum(m, base.double().abs())
        if report:
            _report(f"{what} {tag}", got, r, c, m)
        R.assert_close(got, r, c, m, f"{what} {tag}")


def check_maxpool_fwd(y, tap, x, geom, tag):
    """values and tap bytes [N Ho Wo, C] exactly (a maximum is one of its operands: no arithmetic)"""
    ry, rtap = maxpool_fwd(x, **geom)
    assert y.dtype == x.dtype and torch.equal(y, ry), f"y {tag}: not the window maxima"
    assert tap.dtype == torch.uint8 and torch.equal(tap, rtap), f"tap bytes {tag}: not the first maximum in scan order"


def check_stem_fwd(p, tap, z, mean, invstd, gamma, beta, N, H, W, relu, tag):
    """pooled values and tap bytes exactly against the chain: the forward rounded to the map's dtype, then the pool"""
    rp, rtap = stem_fwd(z, mean, invstd, gamma, beta, N, H, W, relu, z.dtype)
    assert p.dtype == z.dtype and torch.equal(p, rp), f"pooled values {tag}"
    assert tap.dtype == torch.uint8 and torch.equal(tap, rtap), f"tap bytes {tag}"


def check_maxpool_bwd(dx, dy, tap, geom, tag, exact=False):
    """``geom``: the keywords N, H, W, k, stride, pad"""
    ref = maxpool_bwd(dy.double(), tap, **geom)
    if exact:
        assert torch.equal(dx.double(), ref), f"dx {tag}: integer gradients must add exactly"
        return
    R.assert_close(dx, ref, maxpool_bwd(dy.float(), tap, **geom), maxpool_bwd_mag(dy, tap, **geom), f"dx {tag}")


# ---------------------------------------------------------------- mirrors of the host-side partition of conv.hip
WORKGROUPS, PASSES, THREADS = 1024, 4, 256    # bn_parts: about 1024 workgroups, at least 4 passes of the row lanes each
VC_MAX, VC_MIN = 32, 8                        # bn_vc: the divisor search runs from 32 down to 8
FOLD_ABOVE, FOLDS = 256, 64                   # dvt_bn_stats_from_partials folds more than 256 partial rows into 64
CL8_MAX_C = 256                               # bn_finalize_launch: CL = 8 column lanes up to this C, 32 above
ROW_UNROLL = 4                                # kBnU: rows in flight per lane in the row-streaming kernels


def bn_vc_log2(C):
    l = 3
    while l < 5 and (16 << l) <= C:
        l += 1
    return l


def bn_vc(C):
    cv = C >> 3
    if C % 8 or cv <= 0:
        return 1 << bn_vc_log2(C)
    if cv <= VC_MAX:
        return cv
    for v in range(VC_MAX, VC_MIN - 1, -1):
        if cv % v == 0:
            return v
    return 1 << bn_vc_log2(C)


def bn_parts(rows, C):
    """-> (parts, rows_per_block)"""
    vc = bn_vc(C)
    gx = -(-C // (8 * vc))
    nrl = THREADS // vc
    parts = max(1, min(WORKGROUPS // gx, rows // (PASSES * nrl)))
    rpb = -(-rows // parts)
    return -(-rows // rpb), rpb


def row_lanes(C):
    """row lanes of one bn_colstats workgroup"""
    return THREADS // bn_vc(C)


def finalize_cl(C):
    return 8 if C <= CL8_MAX_C else 32


def finalize_tiers(nparts, CL):
    """the loop tiers (16, 8, 4, 1 partial rows per trip) part lane 0 of bn_finalize_kernel<., CL> passes through"""
    PL = 1024 // CL
    p, tiers = 0, []
    while p + 15 * PL < nparts:
        tiers.append(16); p += 16 * PL
    if p + 7 * PL < nparts:
        tiers.append(8); p += 8 * PL
    while p + 3 * PL < nparts:
        tiers.append(4); p += 4 * PL
    while p < nparts:
        tiers.append(1); p += PL
    return tiers


def fold_plan(parts):
    """-> (per_block, blocks with rows, whether a part lane runs the four-way loop) of bn_partial_fold_kernel"""
    per_block = -(-parts // FOLDS)
    return per_block, -(-parts // per_block), per_block > 96


def conv_hip_text():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "data-efficient-video-transformers_amd", "csrc", "conv.hip")) as fh:
        return fh.read()


def conv_hip_constants(text=None):
    """the constants the mirrors restate, read from the text of conv.hip (a KeyError-like assertion if a line moved)"""
    text = conv_hip_text() if text is None else text

    def one(pattern):
        m = re.search(pattern, text, re.S)
        assert m, f"conv.hip no longer has {pattern!r}"
        return tuple(int(g) for g in m.groups())

    parts_body = text[text.index("static int bn_parts("):]
    parts_body = parts_body[:parts_body.index("\n}\n")]
    vc_body = text[text.index("static int bn_vc(int C)"):]
    vc_body = vc_body[:vc_body.index("\n}\n")]
    launch = text[text.index("static void bn_finalize_launch("):]
    launch = launch[:launch.index("\n}\n")]
    return {
        "WORKGROUPS": int(re.search(r"int64_t parts = (\d+) / gx;", parts_body).group(1)),
        "PASSES": int(re.search(r"const int64_t cap = rows / \((\d+) \* nrl\);", parts_body).group(1)),
        "THREADS": int(re.search(r"const int nrl = (\d+) / vc;", parts_body).group(1)),
        "VC": tuple(int(v) for v in re.search(r"for \(int v = (\d+); v >= (\d+); --v\)", vc_body).groups()),
        "VC_DIRECT": int(re.search(r"if \(cv <= (\d+)\) return cv;", vc_body).group(1)),
        "FOLD_ABOVE": one(r"if \(parts > (\d+)\) \{[^\n]*\n[^\n]*fold in place")[0],
        "FOLDS": one(r"const int folds = (\d+);")[0],
        "CL8_MAX_C": int(re.search(r"if \(C <= (\d+)\)\s*\n\s*hipLaunchKernelGGL\(\(bn_finalize_kernel<MODE, 8>\)", launch).group(1)),
        "CL_WIDE": int(re.search(r"else\s*\n\s*hipLaunchKernelGGL\(\(bn_finalize_kernel<MODE, (\d+)>\)", launch).group(1)),
        "ROW_UNROLL": one(r"constexpr int kBnU = (\d+);")[0],
        "VC_LOG2": one(r"int l = (\d+);[^\n]*\n\s*while \(l < (\d+) && \((\d+) << l\) <= C\) \+\+l;"),
        "FOLD_UNROLL": one(r"for \(; p \+ (\d+) < p1; p \+= (\d+)\)"),
        "TIERS": tuple(int(v) for v in re.findall(r"p \+ (\d+) \* PL < nparts", text)),
    }


# ---------------------------------------------------------------- input builders
def randn(shape, dtype, g, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift).to(dtype)


def bn_params(C, g, both_signs=False):
    """gamma, beta f32 [C]: gamma around 1, never near 0; ``both_signs``: every third channel's gamma is negative"""
    gamma = 1.0 + 0.25 * torch.randn(C, generator=g, dtype=torch.float64).clamp(-3, 3)
    if both_signs:
        gamma = torch.where(torch.arange(C) % 3 == 1, -gamma, gamma)
    return gamma.float(), (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float()


def feature_map(rows, C, dtype, g):
    """an ordinary map: columns of differing mean and spread.  Where rows >= 2, rows 0 and 1 of every column are set a whole
    unit apart, so that no column is constant after rounding."""
    shift = torch.randn(C, generator=g, dtype=torch.float64)
    scale = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * scale + shift
    if rows >= 2:
        x[1] = x[0] + 1.0
    return x.to(dtype)


def has_constant_column(x):
    return bool((x.double().max(0).values == x.double().min(0).values).any())


def assert_partials_exact(x, C=None, what="x"):
    """every fp32 partial the mirrored bn_parts row split can form from the integer-valued ``x`` -- any sum of values or of
    squares over rows of one block -- stays below 2^24, so every fp32 addition of the statistics kernels is exact"""
    rows, C = x.shape[0], (x.shape[1] if C is None else C)
    x64 = x.double()
    assert torch.equal(x64, x64.round()), f"{what} is not integer-valued"
    parts, rpb = bn_parts(rows, C)
    pad = parts * rpb - rows
    a = torch.cat([x64.abs(), torch.zeros(pad, x.shape[1], dtype=torch.float64)]).view(parts, rpb, -1)
    worst = max(float(a.sum(1).max()), float((a * a).sum(1).max()))
    assert worst < 2 ** 24, f"a BatchNorm partial of {what} reaches {worst} >= 2^24"
    return worst


def integer_map(rows, C, dtype, g, offset=True):
    """integer-valued columns, exact in every dtype (|x| <= 103 < 2^8): the even columns have mean 100 and spread +-3 (with
    ``offset``), the odd ones mean 0 and spread +-3.  A one-pass variance formed in fp32 from the mean-100 columns' totals
    (E[x^2] = 10^4 against a variance of 4) is lost to rounding; formed in double from exact sums it is exact.  Rows 0 and
    1 differ, so no column is constant."""
    x = torch.randint(-3, 4, (rows, C), generator=g).double()
    if rows >= 2:
        x[0], x[1] = -3.0, 3.0
    if offset:
        x[:, 0::2] += 100.0
    out = x.to(dtype)
    assert torch.equal(out.double(), x) and torch.equal((out.float() * out.float()).double(), x * x)
    assert_partials_exact(out)
    return out


def integer_grad(rows, C, dtype, g):
    """integer-valued dy in [-3, 3]"""
    dy = torch.randint(-3, 4, (rows, C), generator=g).double().to(dtype)
    assert_partials_exact(dy, what="dy")
    return dy


def integer_partials(parts, C, g, n=4):
    """synthetic partial rows [parts + FOLDS, 2, C] f32 (the tail is where the fold writes; it starts as NaN) of ``n`` rows
    each, from the values of integer_map -> (partial, rows, mean64, var64).  Every fold block's sums stay below 2^24."""
    v = torch.randint(-3, 4, (parts, n, C), generator=g).double()
    v[0, 0], v[0, 1] = -3.0, 3.0                             # (no column constant even at parts = 1)
    v[:, :, 0::2] += 100.0
    partial = torch.full((parts + FOLDS, 2, C), math.nan, dtype=torch.float32)
    partial[:parts, 0] = v.sum(1).float()
    partial[:parts, 1] = (v * v).sum(1).float()
    rows = parts * n
    if parts > FOLD_ABOVE:
        per_block = fold_plan(parts)[0]
        assert per_block * n * 104.0 ** 2 < 2 ** 24, "a fold block's sum of squares is not exact in fp32"
    flat = v.reshape(rows, C)
    mean64 = flat.sum(0) / rows
    var64 = (flat * flat).sum(0) / rows - mean64 * mean64
    return partial, rows, mean64, var64


# ---- a ReLU mask recomputed from z
# An element whose pre-activation a = (z - mean) invstd gamma + beta is within rounding of zero may be decided either way
# by a correct kernel, so the inputs have none.  The kernels evaluate a in fp32 in one of two orders: fma((z - mean) *
# invstd, gamma, beta) (fp32 maps, and the scalar kernels) or the folded fma(z, s, t) with s = invstd * gamma and t =
# fma(-mean, s, beta) (16-bit maps).  With u = ulp32(max(|z s|, |t|, |mean s|, |beta|)) -- the largest magnitude either
# order forms on its way -- the first is off a by at most 2 u (the difference, the product, the fma) and the second by at
# most 3 u (s, t, the fma), so MASK_MARGIN_ULPS = 16 of them leaves a factor of five.  (Near a = 0, |z s| and |t| are equal
# to within |a|, and |mean s| <= |t| + |beta|: the unit is the ulp of max(|z s|, |t|) wherever beta does not
# dominate t, and the larger of the two where it does.)  A padded channel of a channel-padded layer (gamma = beta = 0) is
# exactly zero in every evaluation and decided "off" by all of them: it is not counted.
MASK_MARGIN_ULPS = 16


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 tensors: the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def mask_margin(z, mean, invstd, gamma, beta):
    """-> (a in float64, the margin per element)"""
    z64, s = z.double(), invstd.double() * gamma.double()
    t = beta.double() - mean.double() * s
    mag = torch.maximum((z64 * s).abs(), torch.maximum(t.abs(), torch.maximum((mean.double() * s).abs(), beta.double().abs())).expand_as(z64))
    return z64 * s + t, MASK_MARGIN_ULPS * R.ulp32(mag)


def affine_both_orders(z, mean, invstd, gamma, beta):
    """the two fp32 evaluations of the pre-activation the kernels use -> (fp32 order, folded order)"""
    zf = z.float()
    first = fma32((zf - mean) * invstd, gamma.expand_as(zf), beta.expand_as(zf))
    s = invstd * gamma
    t = fma32(-mean, s, beta)
    return first, fma32(zf, s.expand_as(zf), t.expand_as(zf))


def inside_mask_margin(z, mean, invstd, gamma, beta):
    """how many elements are inside the margin, or are decided differently from float64 by one of the two orders"""
    a, margin = mask_margin(z, mean, invstd, gamma, beta)
    first, folded = affine_both_orders(z, mean, invstd, gamma, beta)
    live = ~((gamma == 0) & (beta == 0)).expand_as(a)
    return int((((a.abs() < margin) & live) | ((first > 0) != (a > 0)) | ((folded > 0) != (a > 0))).sum())


def clear_mask_margin(z, mean, invstd, gamma, beta):
    """z with every element inside the margin moved, a step of its dtype at a time, away from the zero of a"""
    z = z.clone()
    s = invstd.double() * gamma.double()
    for _ in range(64):
        a, margin = mask_margin(z, mean, invstd, gamma, beta)
        near = (a.abs() < margin) & ~((gamma == 0) & (beta == 0)).expand_as(a)
        if not near.any():
            break
        up = ((a >= 0) == (s > 0).expand_as(a))                      # the direction in which |a| grows
        inf = torch.tensor(math.inf, dtype=z.dtype)
        moved = torch.where(up, torch.nextafter(z, inf), torch.nextafter(z, -inf))
        z = torch.where(near, moved, z)
    assert inside_mask_margin(z, mean, invstd, gamma, beta) == 0
    return z


# ---- the fused stem's maps
def stem_params(C, g):
    """mean, invstd, gamma, beta f32 [C] on dyadic grids -- mean in quarters, invstd and |gamma| powers of two from 1/2 to 2,
    beta an odd number of 32nds, gamma of both signs -- so that with z in quarters (stem_map) the pre-activation is an odd
    number of 32nds below 2^4: exact in fp32 in either order of evaluation (nine bits), never zero.  A correct kernel's y
    is then the float64 y rounded once to the dtype, its pooled values and taps are THE values and taps of the reference,
    and no mask bit is in doubt (|a| >= 2^-5 against a margin of 16 ulp32(16) = 2^-15)."""
    pick = lambda vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (C,), generator=g)]
    mean = pick([-1.0, -0.5, -0.25, 0.0, 0.25, 0.75])
    invstd = pick([0.5, 1.0, 2.0])
    gamma = pick([0.5, 1.0, 2.0]) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    beta = (2.0 * torch.randint(-16, 16, (C,), generator=g).double() + 1.0) / 32.0
    return mean.float(), invstd.float(), gamma.float(), beta.float()


def stem_map(rows, C, dtype, g):
    """z in quarters, |z| <= 2: few distinct values, so windows tie often"""
    return (torch.randint(-8, 9, (rows, C), generator=g).double() / 4.0).to(dtype)


def tie_map(rows, C, dtype, g, p=0.3):
    """zeros and ones"""
    return (torch.rand(rows, C, generator=g) < p).to(dtype)
