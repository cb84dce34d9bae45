"""Exact results of every kernel that mixes 16x16x32 and 16x16x16 MFMAs on one accumulator (tools/check_mfma_hazards.py).

The hardware does not interlock a dependent accumulate across the two opcodes; a missing wait leaves one k-step out of the
sum (profiles/r06_mfma_shape_hazard.md).  On random data a tolerance test catches that only sometimes.  Here the operands
are integers on which every k-step of every tap adds a nonzero amount to every interior output and every sum is exact
(tests/mfma_exact.py), so the output must equal a float64 convolution of the same operands bit for bit.  The cases are
the rows of tests/test_isa_hazards.py::MIXING_COVERAGE, which fails when a mixing kernel of the library has none."""
import pytest
import torch

from tests import mfma_exact as X

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# (N, T, H, W) per window-forward instantiation: (position blocks per wave, pipelined) as dvt_conv3x1_fwd_plan reports it
WINDOW_CASES = {
    "pipe1": ((3, 2, 4, 4), (1, True)),
    "pipe2": ((3, 4, 4, 4), (2, True)),
    "pipe3": ((3, 6, 4, 4), (3, True)),
    "plain4": ((3, 64, 2, 1), (4, False)),
    "plain5": ((3, 10, 4, 4), (5, False)),
    "plain6": ((3, 64, 3, 1), (6, False)),
}
# (Cin, Cout, N, H, W) per streamed 3x3 instantiation (the 288 -> 128 pair launches the 288 -> 64 kernel once per half)
STREAM_CASES = {
    "144to64": (144, 64, 2, 13, 20),
    "288to128": (288, 128, 2, 13, 20),
}


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", list(WINDOW_CASES))
def test_window_forward_exact(device, case, dname):
    """dvt_conv3x1_fwd (144 -> 64, (3, 1) temporal taps) at every block count of both forms, no virtual BatchNorm."""
    from dvt_amd import ops
    dtype = DTYPES[dname]
    (N, T, H, W), form = WINDOW_CASES[case]
    Lp = H * W
    assert ops.conv3x1_fwd_plan(N, T, Lp, dtype) == form
    x = X.one_hot_input(N * T * Lp, 144, X.WINDOW_RANGES, seed=T * 100 + Lp)
    w = X.window_weights()
    ref = torch.nn.functional.conv2d(x.view(N, T, Lp, 144).permute(0, 3, 1, 2), w, None, 1, (1, 0))
    ref = ref.permute(0, 2, 3, 1).reshape(-1, 64)
    assert ref.max() <= 120 and ref.min() >= 0
    xd = x.to(dtype).cuda()
    wp = ops.conv_weight_pack(w.float().cuda(), ops.conv2d_implicit_k(144, 64, (3, 1)), dtype)
    assert ops.conv3x1_fwd_supported(xd, wp, N, T, Lp, 144, 64)
    y = ops.conv3x1_fwd(xd, wp, N, T, Lp)
    got = y.double().cpu()
    bad = (got != ref).nonzero()
    assert torch.equal(got, ref), f"{bad.shape[0]} outputs differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_stream_conv3x3_exact(device, case, dname):
    """dvt_conv3x3_stream on the 48-channel-chunk instantiations, no residual."""
    from dvt_amd import ops
    dtype = DTYPES[dname]
    Cin, Cout, N, H, W = STREAM_CASES[case]
    x = X.one_hot_input(N * H * W, Cin, X.stream_ranges(Cin), seed=Cin + H)
    w = X.stream_weights(Cin, Cout)
    ref = torch.nn.functional.conv2d(x.view(N, H, W, Cin).permute(0, 3, 1, 2), w, None, 1, 1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert ref.max() <= 9 * len(X.stream_ranges(Cin)) + 1
    xd = x.to(dtype).cuda()
    wp = ops.conv_weight_pack(w.float().cuda(), 9 * Cin, dtype)
    assert ops.conv3x3_stream_supported(xd, wp, N, H, W, Cin, Cout)
    y = ops.conv3x3_stream(xd, wp, N, H, W, Cin, Cout)
    got = y.double().cpu()
    bad = (got != ref).nonzero()
    assert torch.equal(got, ref), f"{bad.shape[0]} outputs differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
