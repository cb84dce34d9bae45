"""Integer operands on which an implicit-GEMM convolution kernel cannot be subtly wrong unseen: for the exact tests of the
convolution forms of gemm_dma_kernel (tests/test_gpu_conv_exact.py) and the CPU proof that they are sensitive
(tests/test_conv_coverage.py).  The idea of tests/gemm_exact.py, whose helpers are reused, carried to the gathered operand.

Forward / data gradient: y[n, ho, wo, co] = sum_{ki, kj, c} x[n, ho*sh - ph + ki, wo*sw - pw + kj, c] w[co, c, ki, kj].
  * the map x is sparse along the channels: per pixel and per 16-wide channel range (the 8 channels of the stem form are one
    range) exactly one nonzero, of magnitude 1 or 2, at a pseudo-random position;
  * the weights are dense, magnitudes 1, 2, 3, with the sign of their (tap, channel range) -- it flips every two ranges
    along the reduction, so no 32-wide k-step cancels itself and the sums stay small;
so every product, partial sum, slab and BatchNorm partial is a small integer, exact in fp32 in any order of addition; every
in-bounds (tap, channel range) adds a nonzero amount to every output pixel and column, a padded one adds exactly zero (a
border pixel's value tells which taps were taken); pixels, channels and columns all differ, so a shifted, repeated or
mis-scattered row or fragment changes the result.  Reductions of more than 64 ranges take magnitudes 1 (map) and 1, 2
(weights) so that the outputs stay exact in bf16 (`check_bound`, asserted on the reference).

Weight gradient: dW[co, c, ki, kj] = sum_{n, ho, wo} dz[n, ho, wo, co] x[n, ho*sh - ph + ki, wo*sw - pw + kj, c]: the
reduction runs over output pixels, so the sparse operand is dz ALONG THE PIXEL AXIS (per column and 16 pixels one nonzero)
and the map is dense: every 32- / 64-pixel k-tile counts, the ragged last one included.

The hand-written LDS-window kernels (tests/test_gpu_window_conv_exact.py, tests/test_window_conv_coverage.py) split the
reduction otherwise -- 32-channel steps, 32 + 16 in 48-channel chunks, a whole filter row of the stem --: kstep_operands keeps
the map and gives the weights the sign of the KERNEL's k-step, so that no step cancels itself.

The references are torch.nn.functional.conv2d in float64 and its two adjoints written out tap by tap in float64.
"""
import torch
import torch.nn.functional as TF

from tests import gemm_exact as X


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H, W, k, stride, pad, trim_w=0):
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1 - trim_w


def channel_ranges(C):
    """the 16-wide channel ranges of a C-channel map (the last may be short; C == 8: one range)"""
    return [(lo, min(C, lo + 16)) for lo in range(0, C, 16)]


def _range_signs(taps, C):
    """[taps, C] +-1: the sign of reduction range r = tap * ranges + j flips every two ranges"""
    rs = channel_ranges(C)
    s = torch.ones(taps, C, dtype=torch.float64)
    for t in range(taps):
        for j, (lo, hi) in enumerate(rs):
            if ((t * len(rs) + j) // 2) % 2:
                s[t, lo:hi] = -1.0
    return s


def sparse_map(rows, C, seed, deep=False):
    """[rows, C] float64 >= 0: one nonzero (1 or 2; deep: 1) per row and channel range"""
    x = X.sparse_rows(rows, C, seed, chunk=min(16, C)).abs()
    return x.clamp(max=1.0) if deep else x


def signed_weights(Cout, C, kh, kw, seed, deep=False):
    """[Cout, C, kh, kw] float64: magnitudes 1..3 (deep: 1..2), sign by (tap, channel range)"""
    taps = kh * kw
    w = X.dense(Cout, taps * C, seed).view(Cout, taps, C)
    if deep:
        w = w.clamp(max=2.0)
    w = w * _range_signs(taps, C).unsqueeze(0)
    return w.permute(0, 2, 1).reshape(Cout, C, kh, kw).contiguous()


def is_deep(C, kh, kw):
    return kh * kw * len(channel_ranges(C)) > 64


def forward_operands(N, C, H, W, Cout, k, seed):
    """-> (x [N, H, W, C], w [Cout, C, kh, kw]) float64"""
    kh, kw = pair(k)
    deep = is_deep(C, kh, kw)
    return sparse_map(N * H * W, C, seed, deep).view(N, H, W, C), signed_weights(Cout, C, kh, kw, seed + 1, deep)


def kstep_signs(kh, kw, C, ranges, tap_group=None):
    """[kh * kw, C] +-1 for a kernel whose k-step is (tap group, channel range of `ranges`): the sign of step
    group * len(ranges) + j flips every two steps, and is constant over a step, so no k-step cancels itself.  tap_group(ki, kj)
    joins taps that share a k-step (the stem kernel: a whole filter row); default: every tap its own."""
    s = torch.ones(kh * kw, C, dtype=torch.float64)
    for tap in range(kh * kw):
        grp = tap if tap_group is None else tap_group(tap // kw, tap % kw)
        for j, (lo, hi) in enumerate(ranges):
            if ((grp * len(ranges) + j) // 2) % 2:
                s[tap, lo:hi] = -1.0
    return s


def kstep_operands(N, C, H, W, Cout, k, seed, ranges, tap_group=None, valid=None, deep=None):
    """forward_operands for the hand-written window kernels, whose k-steps are not 16 channels wide: the map keeps one nonzero
    per pixel and 16-channel range (so every 16-byte slot matters), the weights take the sign of their k-step (kstep_signs).
    valid: channels that exist (the rest of the C stored ones are zero in the map AND in the weights: a zero-padded layer).
    -> (x [N, H, W, C], w [Cout, C, kh, kw]) float64"""
    kh, kw = pair(k)
    valid = valid or C
    assert ranges[-1][1] == valid and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    deep = is_deep(valid, kh, kw) if deep is None else deep
    x = torch.zeros(N * H * W, C, dtype=torch.float64)
    x[:, :valid] = sparse_map(N * H * W, valid, seed, deep)
    w = X.dense(Cout, kh * kw * C, seed + 1).view(Cout, kh * kw, C)
    if deep:
        w = w.clamp(max=2.0)
    w = w * kstep_signs(kh, kw, C, ranges, tap_group).unsqueeze(0)
    w[:, :, valid:] = 0.0
    return x.view(N, H, W, C), w.permute(0, 2, 1).reshape(Cout, C, kh, kw).contiguous()


def adjoint_weights(wd):
    """the layer's parameter whose DATA GRADIENT is the convolution with wd [Cin, Cout, kh, kw] (stride 1, same padding):
    w[co, ci, ki, kj] = wd[ci, co, kh - 1 - ki, kw - 1 - kj]"""
    return wd.flip(2, 3).permute(1, 0, 2, 3).contiguous()


def wgrad_operands(N, C, H, W, Cout, k, stride, pad, seed, trim_w=0):
    """-> (x [N, H, W, C] dense 1..3, dz [N, Ho, Wo, Cout] sparse along the pixel axis) float64"""
    Ho, Wo = out_hw(H, W, k, stride, pad, trim_w)
    rows = N * Ho * Wo
    x = X.dense(N * H * W, C, seed).view(N, H, W, C)
    dz = X.sparse_rows(Cout, rows, seed + 1, chunk=16).t().contiguous().view(N, Ho, Wo, Cout)
    return x, dz


def pack_weights(w, K):
    """w [Cout, C, kh, kw] -> the forward operand [Cout, K]: column (ki * kw + kj) * C + c, zeros beyond kh * kw * C"""
    Cout, C, kh, kw = w.shape
    wp = torch.zeros(Cout, K, dtype=w.dtype)
    wp[:, :kh * kw * C] = w.permute(0, 2, 3, 1).reshape(Cout, kh * kw * C)
    return wp


# ---------------------------------------------------------------- float64 references
def conv_ref(x, w, stride, pad, trim_w=0):
    """[N, H, W, C], [Cout, C, kh, kw] -> [N * Ho * Wo, Cout] (torch.nn.functional.conv2d in float64)"""
    assert x.dtype == w.dtype == torch.float64
    y = TF.conv2d(x.permute(0, 3, 1, 2), w, None, pair(stride), pair(pad)).permute(0, 2, 3, 1)
    if trim_w:
        y = y[:, :, :y.shape[2] - trim_w]
    return y.reshape(-1, w.shape[0]).contiguous()


def _padded(x, ph, pw):
    return TF.pad(x, (0, 0, pw, pw, ph, ph))


def tap_view(xp, ki, kj, Ho, Wo, sh, sw):
    """the pixels tap (ki, kj) reads for every output pixel: [N, Ho, Wo, C] of the zero-padded map xp"""
    return xp[:, ki:ki + sh * (Ho - 1) + 1:sh, kj:kj + sw * (Wo - 1) + 1:sw]


def wgrad_ref(x, dz, k, stride, pad):
    """weight adjoint written out: -> dW [Cout, C, kh, kw] float64 (dz [N, Ho, Wo, Cout] fixes Ho, Wo: trim_w included)"""
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    _, Ho, Wo, Cout = dz.shape
    xp = _padded(x, ph, pw)
    dW = torch.zeros(Cout, x.shape[3], kh, kw, dtype=torch.float64)
    for ki in range(kh):
        for kj in range(kw):
            dW[:, :, ki, kj] = torch.einsum("nhwo,nhwc->oc", dz, tap_view(xp, ki, kj, Ho, Wo, sh, sw))
    return dW


def dgrad_ref(dz, w, H, W, stride, pad):
    """input adjoint written out: dz [N, Ho, Wo, Cout], w [Cout, C, kh, kw] -> dx [N * H * W, C] float64"""
    (sh, sw), (ph, pw) = pair(stride), pair(pad)
    Cout, C, kh, kw = w.shape
    N, Ho, Wo, _ = dz.shape
    Hp, Wp = max(H + 2 * ph, kh + sh * (Ho - 1)), max(W + 2 * pw, kw + sw * (Wo - 1))
    dxp = torch.zeros(N, Hp, Wp, C, dtype=torch.float64)
    for ki in range(kh):
        for kj in range(kw):
            tap_view(dxp, ki, kj, Ho, Wo, sh, sw).add_(torch.einsum("nhwo,oc->nhwc", dz, w[:, :, ki, kj]))
    return dxp[:, ph:ph + H, pw:pw + W].reshape(-1, C).contiguous()


def stats_ref(y):
    """column sums and sums of squares of the stored map: [2, Cout] float64"""
    return torch.stack([y.sum(0), (y * y).sum(0)])


def check_stats_bound(y, rows_per_part):
    """every partial row ({sum, sum of squares} of rows_per_part output rows) stays an exact fp32 integer"""
    worst = 0.0
    for r0 in range(0, y.shape[0], rows_per_part):
        blk = y[r0:r0 + rows_per_part]
        worst = max(worst, float(blk.abs().sum(0).max()), float((blk * blk).sum(0).max()))
    assert worst < 2 ** 24, f"a BatchNorm partial reaches {worst} >= 2^24"
    return worst


# ---------------------------------------------------------------- sensitivity (CPU): the faults these operands expose
def tap_range_partial(x, w, stride, pad, ki, kj, lo, hi, trim_w=0):
    """-> (what tap (ki, kj), channels [lo, hi) adds to y [N * Ho * Wo, Cout], in-bounds mask [N * Ho * Wo])"""
    (sh, sw), (ph, pw) = pair(stride), pair(pad)
    Cout, C, kh, kw = w.shape
    N, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W, (kh, kw), stride, pad, trim_w)
    v = tap_view(_padded(x, ph, pw), ki, kj, Ho, Wo, sh, sw)
    inb = tap_view(_padded(torch.ones(N, H, W, 1, dtype=torch.float64), ph, pw), ki, kj, Ho, Wo, sh, sw)
    part = torch.einsum("nhwc,oc->nhwo", v[..., lo:hi], w[:, lo:hi, ki, kj])
    return part.reshape(-1, Cout), inb.reshape(-1) > 0


def im2col(x, k, stride, pad, trim_w=0):
    """the column matrix the kernels never build: [N * Ho * Wo, kh * kw * C] float64, column (ki * kw + kj) * C + c"""
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, k, stride, pad, trim_w)
    xp = _padded(x, ph, pw)
    cols = [tap_view(xp, ki, kj, Ho, Wo, sh, sw).reshape(-1, C) for ki in range(kh) for kj in range(kw)]
    return torch.cat(cols, 1)


def shifted_map(x, dh, dw):
    """the map every gather of which lands one pixel off (zeros shifted in)"""
    out = torch.zeros_like(x)
    H, W = x.shape[1], x.shape[2]
    out[:, max(0, -dh):H - max(0, dh), max(0, -dw):W - max(0, dw)] = x[:, max(0, dh):H - max(0, -dh), max(0, dw):W - max(0, -dw)]
    return out
