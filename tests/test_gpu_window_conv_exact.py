"""Exact results of every LDS-window convolution kernel: the halo-patch 3x3 kernels (conv3x3_c64_kernel, conv3x3_stream_kernel,
conv3x3_c64_wgrad_kernel), the frame-window (3, 1) kernels (conv3x1_c64_kernel, conv3x1_dbn_kernel, conv3x1_wgrad[_pipe]_kernel)
and conv_stem_kernel.  (conv3x1_fwd[_pipe]_kernel and the 144- / 288-channel stream forms mix MFMA shapes and have their plain
cases in tests/test_gpu_mfma_exact.py; the stream forms run here too, with statistics or a residual.)

Each case names the instantiation it was written for and asserts, before launching, that the library's plan query reports it.
Operands are the integers of tests/conv_exact.py (kstep_operands: every k-step of the kernel -- one tap, or one filter row of
the stem, times the channel range of one MFMA -- adds a nonzero integer of one sign to every output whose tap reads inside
the map; weights differ per output channel, tap and channel), so outputs, BatchNorm partial sums and fp32 weight gradients
must equal the float64 reference -- torch.nn.functional.conv2d and its adjoints written out -- bit for bit (torch.equal):
there is no tolerance in this file.  Shapes: per kernel one launch of a few tiles whose last tile of an image is ragged (the
frame-window kernels and the R = 1 tiling of the MB = 1 weight gradient have no ragged tile: a tile is a whole segment / one
row) and a `persist` one with more than BUFFERS x 256 tiles, so that a workgroup of the 256-CU persistent grid runs through
every LDS buffer AND wraps back to the first, and the last round is partial.  tests/test_window_conv_coverage.py ties every kernel symbol of the
family to one of these cases and proves on the CPU that the operands see a missing, doubled or misplaced piece.
"""
import functools

import pytest
import torch

from tests import conv_exact as V
from tests import gemm_exact as X
from tests import mfma_exact as M

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
DTYPES = {"bf16": BF, "fp16": FP}
R64 = [(0, 32), (32, 64)]                       # the k-steps of a 64-channel chunk: two 16x16x32 MFMAs


def stream_kranges(cin):
    """channel ranges of conv3x3_stream_kernel's k-steps: 64-channel chunks as 32 + 32, 48-channel chunks as 32 + 16"""
    return M.stream_ranges(cin) if cin % 48 == 0 else [(c, c + 32) for c in range(0, cin, 32)]


# ---------------------------------------------------------------- cases
# conv3x3_c64_kernel: N, H, W (R = min(256 / W, H) rows per tile)
C64_CASES = {
    "ragged_13x20": (2, 13, 20),                # R = 12: 4 tiles, the second of an image 1 row high
    "ragged_5x56": (1, 5, 56),                  # R = 4: the workload's width, 2 tiles
    "persist_8x8": (520, 8, 8),                 # 520 tiles on 256 workgroups: both patch buffers and back, a partial last round
}
# conv3x3_stream_kernel<., ci, co, 9, 0>: Cin, Cout, N, H, W -> (ci, co, launches)   (R = min(224 / W, H))
STREAM_CASES = {
    "64to144_ragged": ((64, 144, 2, 13, 20), (64, 144, 1)),
    "64to144_persist": ((64, 144, 520, 8, 8), (64, 144, 1)),
    "144to64_ragged": ((144, 64, 2, 13, 20), (144, 64, 1)),
    "144to64_persist": ((144, 64, 520, 8, 8), (144, 64, 1)),
    "128to288_ragged": ((128, 288, 2, 13, 20), (128, 144, 2)),
    "128to288_persist": ((128, 288, 520, 8, 8), (128, 144, 2)),
    "288to128_ragged": ((288, 128, 2, 13, 20), (288, 64, 2)),
    "288to128_persist": ((288, 128, 520, 8, 8), (288, 64, 2)),
}
# conv3x3_stream_kernel<., 64, 144, 3, 0> (dvt_conv3x1_stream): N, T, H, W
STREAM31_CASES = {
    "ragged_5x112": (2, 5, 14, 8),              # segments of 112 pixels, 2 frames per tile: 3 tiles per clip, the last 1 frame
    "persist_5x32": (520, 5, 4, 8),             # 520 tiles
}
# conv3x1_c64_kernel<., NPB>: N, T, H, W -> NPB; every case with the forward and the data-gradient pack
WIN64_CASES = {f"npb{n}_{tag}": ((N, 2 * n, 4, 8), n) for n in range(1, 7) for tag, N in (("few", 3), ("persist", 260))}   # 6 / 520 tiles
# conv_stem_kernel: N, H, Wp (pixel pairs per row); Ho = H / 2, Wo = Wp, R = min(896 / Wo, Ho)
STEM_CASES = {
    "ragged_odd": (2, 26, 75),                  # 13 x 75 outputs (both odd), R = 11: the second tile 2 rows high
    "persist_8x8": (520, 8, 8),
}
# conv3x3_c64_wgrad_kernel<., MB>: N, H, W, Cout -> ((first channel, channels, MB) per launch)
WGRAD33_CASES = {
    "mb4_ragged": ((2, 19, 20, 64), ((0, 64, 4),)),                   # 13 rows per tile: the second tile of an image 6 rows high
    "mb4_persist": ((520, 8, 8, 64), ((0, 64, 4),)),
    "mb5_ragged": ((2, 19, 20, 144), ((0, 64, 4), (64, 80, 5))),       # (the 80-wide group: 11 rows per tile)
    "mb5_persist": ((520, 8, 8, 144), ((0, 64, 4), (64, 80, 5))),
    "mb1_wide_row": ((2, 3, 150, 80), ((0, 64, 4), (64, 16, 1))),      # W = 150: no LDS for 160-byte gradient positions
    "mb1_persist": ((175, 3, 150, 80), ((0, 64, 4), (64, 16, 1))),     # R = 1: 525 tiles
}
# conv3x1_wgrad_kernel / conv3x1_wgrad_pipe_kernel: N, T, H, W -> pipelined
WGRAD31_CASES = {
    "pipe_few": ((3, 2, 4, 4), True),
    "pipe_persist": ((400, 2, 4, 8), True),     # 800 tiles: the three buffer pairs and back to the first
    "plain_few": ((3, 64, 2, 1), False),
    "plain_persist": ((520, 64, 2, 1), False),
}
# dvt_conv3x1_stream_bn_bwd: N, T, H, W -> (kernel, NB): conv3x1_dbn_kernel<., NB, 1 | 2> or conv3x3_stream_kernel<., 64, 144, 3, 1 | 2>
DBN_CASES = {
    "nb2_few": ((2, 2, 8, 8), ("window", 2)),
    "nb2_persist": ((200, 2, 8, 8), ("window", 2)),      # 800 tiles: a workgroup runs 3 or 4, the fourth in the first window again
    "nb4_few": ((2, 4, 8, 8), ("window", 4)),
    "nb4_persist": ((200, 4, 8, 8), ("window", 4)),
    "nb6_few": ((2, 6, 8, 8), ("window", 6)),
    "nb6_persist": ((200, 6, 8, 8), ("window", 6)),
    "stream_ragged": ((2, 5, 14, 8), ("stream", 0)),     # T = 5: no segment of at most 16 pixels makes a multiple of 32 positions
    "stream_persist": ((520, 5, 4, 8), ("stream", 0)),
}


def _seed(*g):
    return sum((i + 3) * int(v) for i, v in enumerate(g))


def _res(y, seed):
    return X.small_ints(tuple(y.shape), -3, 3, seed)


# ---------------------------------------------------------------- CPU float64: operands and references
@functools.lru_cache(maxsize=2)
def build_c64(name):
    N, H, W = C64_CASES[name]
    x, w = V.kstep_operands(N, 64, H, W, 64, 3, _seed(N, H, W), R64)
    y = V.conv_ref(x, w, 1, 1)
    return dict(x=x, w=w, y=y, res=_res(y, _seed(N, H, W) + 5), geom=(N, 64, H, W, 64, 3, 1, 1), ranges=R64, tap_group=None)


@functools.lru_cache(maxsize=2)
def build_stream(name):
    (Cin, Cout, N, H, W), _ = STREAM_CASES[name]
    x, w = V.kstep_operands(N, Cin, H, W, Cout, 3, _seed(N, H, W, Cin), stream_kranges(Cin))
    y = V.conv_ref(x, w, 1, 1)
    return dict(x=x, w=w, y=y, res=_res(y, _seed(N, H, W, Cin) + 5), geom=(N, Cin, H, W, Cout, 3, 1, 1),
                ranges=stream_kranges(Cin), tap_group=None)


@functools.lru_cache(maxsize=2)
def build_stream31(name):
    N, T, H, W = STREAM31_CASES[name]
    x, w = V.kstep_operands(N, 64, T, H * W, 144, (3, 1), _seed(N, T, H, W), R64)
    return dict(x=x, w=w, y=V.conv_ref(x, w, 1, (1, 0)), geom=(N, 64, T, H * W, 144, (3, 1), 1, (1, 0)), ranges=R64, tap_group=None)


R45 = [(0, 32), (32, 45)]                       # the stem's 45 mid planes inside the 64 stored ones


@functools.lru_cache(maxsize=2)
def build_win64(name):
    """the stem's temporal half Conv3d(45, 64, (3, 1, 1)): forward (45 valid input planes of 64) and its data gradient (45
    valid OUTPUT planes: the gradient's padded planes must come out exactly zero)"""
    (N, T, H, W), _ = WIN64_CASES[name]
    Lp, s = H * W, _seed(N, T, H, W)
    x, w = V.kstep_operands(N, 64, T, Lp, 64, (3, 1), s, R45, valid=45)
    y = V.conv_ref(x, w, 1, (1, 0))
    # the data gradient as the convolution it is: dz [., 64] with wd [ci 64 (45 valid), co 64, 3, 1]; its own parameter wg
    dz, wd = V.kstep_operands(N, 64, T, Lp, 64, (3, 1), s + 7, R64)
    wd[45:] = 0.0
    wg = V.adjoint_weights(wd)                                        # [co 64, ci 64 (45 valid), 3, 1]
    dx = V.dgrad_ref(dz, wg, T, Lp, 1, (1, 0))
    return dict(x=x, w=w, y=y, dz=dz, wd=wd, wg=wg, dx=dx, geom=(N, 64, T, Lp, 64, (3, 1), 1, (1, 0)), ranges=R45, tap_group=None)


def _stem_row(ki, kj):
    return ki                                   # one 16x16x32 k-step of conv_stem_kernel is a whole filter row: 4 pairs x 8


@functools.lru_cache(maxsize=2)
def build_stem(name):
    """in the pixel-pair domain: x [N, H, Wp, 8], w [64, 8, 7, 4], stride (2, 1), pad (3, 2), the last output column trimmed"""
    N, H, Wp = STEM_CASES[name]
    x, w = V.kstep_operands(N, 8, H, Wp, 64, (7, 4), _seed(N, H, Wp), [(0, 8)], tap_group=_stem_row)
    return dict(x=x, w=w, y=V.conv_ref(x, w, (2, 1), (3, 2), 1), geom=(N, 8, H, Wp, 64, (7, 4), (2, 1), (3, 2)), ranges=[(0, 8)],
                tap_group=_stem_row, trim_w=1)


@functools.lru_cache(maxsize=2)
def build_wgrad33(name):
    (N, H, W, Cout), _ = WGRAD33_CASES[name]
    x, dz = V.wgrad_operands(N, 64, H, W, Cout, 3, 1, 1, _seed(N, H, W, Cout))
    dW = V.wgrad_ref(x, dz, 3, 1, 1)
    return dict(x=x, dz=dz, dW=dW, prior=X.small_ints(tuple(dW.shape), -4, 4, _seed(N, H, W, Cout) + 9), k=3, pad=1)


@functools.lru_cache(maxsize=2)
def build_wgrad31(name):
    (N, T, H, W), _ = WGRAD31_CASES[name]
    x, dz = V.wgrad_operands(N, 144, T, H * W, 64, (3, 1), 1, (1, 0), _seed(N, T, H, W))
    dW = V.wgrad_ref(x, dz, (3, 1), 1, (1, 0))
    return dict(x=x, dz=dz, dW=dW, prior=X.small_ints(tuple(dW.shape), -4, 4, _seed(N, T, H, W) + 9), k=(3, 1), pad=(1, 0))


@functools.lru_cache(maxsize=2)
def build_dbn(name):
    """mean 0, invstd 1, gamma a power of two, beta an integer: xhat = z, the ReLU mask is z * gamma + beta > 0 and cuts about
    half; d = the data gradient of the temporal convolution (never stored by the kernels) -> dgamma = sum dzm z, dbeta = sum
    dzm, eval-mode dz = gamma dzm"""
    (N, T, H, W), _ = DBN_CASES[name]
    Lp, s = H * W, _seed(N, T, H, W)
    dy, wd = V.kstep_operands(N, 64, T, Lp, 144, (3, 1), s, R64, deep=True)     # (small d: gamma * d stays exact in bf16)
    wg = V.adjoint_weights(wd)                                                  # the layer's parameter [64, 144, 3, 1]
    d = V.conv_ref(dy, wd, 1, (1, 0))
    z = X.small_ints(tuple(d.shape), -3, 3, s + 3)
    c = torch.arange(144)
    gamma, beta = 2.0 ** ((c % 4) - 1).double(), ((c % 3) - 1).double()
    mask = z * gamma + beta > 0
    dzm = torch.where(mask, d, torch.zeros_like(d))
    return dict(dy=dy, wd=wd, wg=wg, d=d, z=z, gamma=gamma, beta=beta, mask=mask, dzm=dzm, dgamma=(dzm * z).sum(0), dbeta=dzm.sum(0),
                dz_eval=gamma * dzm, dz_eval_norelu=gamma * d, dgamma_norelu=(d * z).sum(0), dbeta_norelu=d.sum(0),
                geom=(N, 64, T, Lp, 144, (3, 1), 1, (1, 0)), ranges=R64, tap_group=None)


# ---------------------------------------------------------------- comparisons
def assert_exact(got, want, what):
    got = got.double().cpu()
    diff = (got != want) | torch.isnan(got)
    bad = int(diff.sum())
    print(f"{what}: {bad} of {want.numel()} elements differ")
    assert torch.equal(got, want), f"{what}: {bad} of {want.numel()} elements differ, first {diff.nonzero()[:8].tolist()}"


# what one fp32 partial row can hold at most: the pixels of a tile (conv3x3_c64: R W <= 256, conv3x3_stream: 224, conv_stem: 896,
# conv3x1_c64: T S <= 192) times the tiles of a workgroup -- every case here has at most 3 x 256 tiles
PARTIAL_ROWS = {"c64": 3 * 256, "stream": 3 * 224, "stem": 3 * 896, "win64": 3 * 192}


def check_partial_bound(y, fam):
    """every fp32 partial row is exact whatever rows it holds and in any order: PARTIAL_ROWS[fam] squares of the largest output
    stay below 2^24 (the float64 sum over the partial rows is exact anyway)"""
    worst = min(PARTIAL_ROWS[fam], y.shape[0]) * float(y.abs().max()) ** 2
    assert worst < 2 ** 24, f"a BatchNorm partial row may reach {worst} >= 2^24"


def assert_stats(partial, parts, y, what, fam):
    """the float64 sum over the partial rows is the exact column sum / sum of squares of the stored output, both rows, every
    channel"""
    Cout = y.shape[1]
    check_partial_bound(y, fam)
    assert parts > 0
    got = partial.view(-1)[:parts * 2 * Cout * 4].view(torch.float32).double().cpu().view(parts, 2, Cout).sum(0)   # (a byte buffer)
    want = V.stats_ref(y)
    diff = got != want
    assert torch.equal(got, want), f"{what}: {int(diff.sum())} of {2 * Cout} statistics differ, first {diff.nonzero()[:8].tolist()}"


def _dev(t, dtype):
    return t.to(dtype).cuda().contiguous()


def _pack(ops, w, dtype):
    Cout, C, kh, kw = w.shape
    return ops.conv_weight_pack(w.float().cuda(), kh * kw * C, dtype)


# ---------------------------------------------------------------- forward / data-gradient kernels
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(C64_CASES))
def test_conv3x3_c64_exact(device, name, dname):
    from dvt_amd import ops
    dtype, (N, H, W), b = DTYPES[dname], C64_CASES[name], build_c64(name)
    X.check_bound(b["y"], dtype)
    X.check_bound(b["y"] + b["res"], dtype)
    x, wp = _dev(b["x"].reshape(-1, 64), dtype), _pack(ops, b["w"], dtype)
    assert ops.conv3x3_c64_supported(x, wp, N, H, W)
    assert_exact(ops.conv3x3_c64(x, wp, N, H, W), b["y"], f"{name} {dname}")
    y, partial, parts = ops.conv3x3_c64(x, wp, N, H, W, want_stats=True)
    assert_exact(y, b["y"], f"{name} {dname} with statistics")
    assert_stats(partial, parts, b["y"], f"{name} {dname}", "c64")
    y, partial, parts = ops.conv3x3_c64(x, wp, N, H, W, want_stats=True, residual=_dev(b["res"], dtype))
    assert_exact(y, b["y"] + b["res"], f"{name} {dname} with a residual")
    assert_stats(partial, parts, b["y"] + b["res"], f"{name} {dname} with a residual", "c64")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_conv3x3_stream_exact(device, name, dname):
    from dvt_amd import ops
    dtype, ((Cin, Cout, N, H, W), inst), b = DTYPES[dname], STREAM_CASES[name], build_stream(name)
    assert ops.conv3x3_stream_plan(N, H, W, Cin, Cout, dtype) == inst
    X.check_bound(b["y"], dtype)
    x, wp = _dev(b["x"].reshape(-1, Cin), dtype), _pack(ops, b["w"], dtype)
    assert ops.conv3x3_stream_supported(x, wp, N, H, W, Cin, Cout)
    assert_exact(ops.conv3x3_stream(x, wp, N, H, W, Cin, Cout), b["y"], f"{name} {dname}")
    if Cout % 144 == 0:                                     # statistics come with the wide output, the residual with the narrow one
        y, partial, parts = ops.conv3x3_stream(x, wp, N, H, W, Cin, Cout, want_stats=True)
        assert_exact(y, b["y"], f"{name} {dname} with statistics")
        assert_stats(partial, parts, b["y"], f"{name} {dname}", "stream")
    else:
        X.check_bound(b["y"] + b["res"], dtype)
        y = ops.conv3x3_stream(x, wp, N, H, W, Cin, Cout, residual=_dev(b["res"], dtype))
        assert_exact(y, b["y"] + b["res"], f"{name} {dname} with a residual")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(STREAM31_CASES))
def test_conv3x1_stream_exact(device, name, dname):
    from dvt_amd import ops
    dtype, (N, T, H, W), b = DTYPES[dname], STREAM31_CASES[name], build_stream31(name)
    X.check_bound(b["y"], dtype)
    x, wp = _dev(b["x"].reshape(-1, 64), dtype), _pack(ops, b["w"], dtype)
    assert ops.conv3x1_stream_supported(x, wp, N, T, H * W, 64, 144)
    assert_exact(ops.conv3x1_stream(x, wp, N, T, H * W, 64, 144), b["y"], f"{name} {dname}")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(WIN64_CASES))
def test_conv3x1_c64_exact(device, name, dname):
    from dvt_amd import ops
    dtype, ((N, T, H, W), npb), b = DTYPES[dname], WIN64_CASES[name], build_win64(name)
    Lp = H * W
    assert ops.conv3x1_c64_plan(N, T, Lp, dtype) == npb
    X.check_bound(b["y"], dtype)
    X.check_bound(b["dx"], dtype)
    x, wp = _dev(b["x"].reshape(-1, 64), dtype), _pack(ops, b["w"], dtype)
    assert ops.conv3x1_fwd_supported(x, wp, N, T, Lp, 64, 64)
    assert_exact(ops.conv3x1_fwd(x, wp, N, T, Lp), b["y"], f"{name} {dname} forward pack")
    y, partial, parts = ops.conv3x1_fwd(x, wp, N, T, Lp, want_stats=True)
    assert_exact(y, b["y"], f"{name} {dname} forward pack with statistics")
    assert_stats(partial, parts, b["y"], f"{name} {dname}", "win64")
    # the data-gradient pack of the layer's own parameter (dvt_conv_weight_pack_dgrad): planes 45 .. 63 exactly zero
    wd = ops.conv_weight_pack_dgrad(b["wg"].float().cuda(), dtype)
    dx = ops.conv3x1_fwd(_dev(b["dz"].reshape(-1, 64), dtype), wd, N, T, Lp)
    assert_exact(dx, b["dx"], f"{name} {dname} data-gradient pack")
    assert float(b["dx"][:, 45:].abs().max()) == 0.0 and float(dx[:, 45:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(STEM_CASES))
def test_conv_stem_exact(device, name, dname):
    from dvt_amd import ops
    dtype, (N, H, Wp), b = DTYPES[dname], STEM_CASES[name], build_stem(name)
    X.check_bound(b["y"], dtype)
    x = _dev(b["x"].reshape(-1, 8), dtype)
    wp = ops.conv_weight_pack(b["w"].float().cuda(), ops.conv2d_implicit_k(8, 64, (7, 4)), dtype)
    assert ops.conv_stem7_supported(x, wp, N, H, Wp)
    assert_exact(ops.conv_stem7(x, wp, N, H, Wp), b["y"], f"{name} {dname}")
    y, partial, parts = ops.conv_stem7(x, wp, N, H, Wp, want_stats=True)
    assert_exact(y, b["y"], f"{name} {dname} with statistics")
    assert_stats(partial, parts, b["y"], f"{name} {dname}", "stem")


# ---------------------------------------------------------------- weight-gradient kernels
def _wgrad_three_ways(run, b, what):
    """into a NaN-filled dw; accumulated onto an integer dw; deferred + flushed: all three the float64 gradient"""
    from dvt_amd import ops
    dW, prior = b["dW"], b["prior"]
    assert float(dW.abs().max()) + 4 < 2 ** 24
    dw = torch.full(tuple(dW.shape), float("nan"), device="cuda")
    run(dw)
    assert_exact(dw, dW, f"{what} into NaN")
    acc = prior.float().cuda()
    run(acc, accumulate=True)
    assert_exact(acc, prior + dW, f"{what} accumulated")
    dw2 = torch.full(tuple(dW.shape), float("nan"), device="cuda")
    pend = run(dw2, defer_reduce=True)
    assert pend is not None and pend.valid
    ops.splitk_reduce_pending(pend)
    torch.cuda.synchronize()
    assert_exact(dw2, dW, f"{what} deferred and flushed")
    assert torch.equal(dw2, dw) and torch.equal(acc.double().cpu() - prior, dw.double().cpu())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(WGRAD33_CASES))
def test_conv3x3_c64_wgrad_exact(device, name, dname):
    from dvt_amd import ops
    dtype, ((N, H, W, Cout), launches), b = DTYPES[dname], WGRAD33_CASES[name], build_wgrad33(name)
    assert ops.conv3x3_c64_wgrad_plan(N, H, W, Cout, dtype) == launches
    x, dz = _dev(b["x"].reshape(-1, 64), dtype), _dev(b["dz"].reshape(-1, Cout), dtype)
    assert ops.conv3x3_c64_wgrad_supported(x, dz, N, H, W, Cout)
    _wgrad_three_ways(lambda dw, **kw: ops.conv3x3_c64_wgrad(x, dz, N, H, W, dw, Cout=Cout, **kw), b, f"{name} {dname}")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(WGRAD31_CASES))
def test_conv3x1_wgrad_exact(device, name, dname):
    from dvt_amd import ops
    dtype, ((N, T, H, W), pipelined), b = DTYPES[dname], WGRAD31_CASES[name], build_wgrad31(name)
    Lp = H * W
    assert ops.conv3x1_wgrad_plan(N, T, Lp, dtype) is pipelined
    x, dz = _dev(b["x"].reshape(-1, 144), dtype), _dev(b["dz"].reshape(-1, 64), dtype)
    assert ops.conv3x1_wgrad_supported(x, dz, N, T, Lp, 144, 64)
    _wgrad_three_ways(lambda dw, **kw: ops.conv3x1_wgrad(x, dz, N, T, Lp, dw, **kw), b, f"{name} {dname}")


# ---------------------------------------------------------------- the fused BatchNorm backward
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(DBN_CASES))
def test_conv3x1_bn_bwd_exact(device, name, dname):
    """MODE 1 through dgamma / dbeta (accumulate = 0), MODE 2 in eval mode: gamma * invstd * dzm.  (The training-mode
    correction divides by the row count, no power of two for the NB = 6 and stream geometries: it stays with the tolerance tests
    test_fused_mid_batchnorm_backward_against_fp32_autograd and
    test_temporal_data_gradient_with_the_mid_batchnorm_backward_fused of tests/test_gpu_cnn.py.)"""
    from dvt_amd import ops
    dtype, ((N, T, H, W), plan), b = DTYPES[dname], DBN_CASES[name], build_dbn(name)
    Lp = H * W
    assert ops.conv3x1_stream_bn_bwd_plan(N, T, Lp, dtype) == plan
    for k in ("d", "dz_eval", "dz_eval_norelu"):
        X.check_bound(b[k], dtype)
    assert float((b["dzm"] * b["z"]).abs().sum(0).max()) < 2 ** 24 and float((b["d"] * b["z"]).abs().sum(0).max()) < 2 ** 24
    dy, z = _dev(b["dy"].reshape(-1, 64), dtype), _dev(b["z"], dtype)
    wd = ops.conv_weight_pack_dgrad(b["wg"].float().cuda(), dtype)
    assert ops.conv3x1_stream_supported(dy, wd, N, T, Lp, 64, 144)
    mean, invstd = torch.zeros(144, device="cuda"), torch.ones(144, device="cuda")
    gamma, beta = b["gamma"].float().cuda(), b["beta"].float().cuda()
    dz, dg, db = ops.conv3x1_stream_bn_bwd(dy, wd, z, (mean, invstd, gamma, beta, 0, True), N, T, Lp, False)
    assert_exact(dg, b["dgamma"], f"{name} {dname} dgamma")
    assert_exact(db, b["dbeta"], f"{name} {dname} dbeta")
    assert_exact(dz, b["dz_eval"], f"{name} {dname} eval-mode dz")
    dz, dg, db = ops.conv3x1_stream_bn_bwd(dy, wd, z, (mean, invstd, gamma, beta, 0, False), N, T, Lp, False)
    assert_exact(dg, b["dgamma_norelu"], f"{name} {dname} dgamma without the ReLU")
    assert_exact(db, b["dbeta_norelu"], f"{name} {dname} dbeta without the ReLU")
    assert_exact(dz, b["dz_eval_norelu"], f"{name} {dname} eval-mode dz without the ReLU")
