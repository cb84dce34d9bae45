"""Exact integer tests of the layer-1 inference kernels of R(2+1)D-18 (csrc/conv2p1d_l1.hip, dvt_conv2p1d_l1), in the style
of tests/mfma_exact.py: the input has exactly one 1 per pixel and k-step channel range (at a pixel-dependent channel), the
weights are constant over a range, a distinct small positive integer per (output channel, tap, range).  Every k-step of
every tap then adds its own nonzero weight to every output whose tap reads inside the map, the sums are integers <= 256
(exact in bf16 and fp16), and a dropped or doubled k-step changes the output.  The epilogue uses power-of-two scales and
integer shifts / residuals, so the whole result is exact and compared bit for bit."""
import pytest
import torch
import torch.nn.functional as TF

from tests.mfma_exact import one_hot_input

pytestmark = pytest.mark.gpu

# (name, Cin, Cout, k, pad, channel ranges of one k-step)
HALVES = {
    "spatial": (64, 144, (1, 3, 3), (0, 1, 1), [(0, 32), (32, 64)]),
    "temporal": (144, 64, (3, 1, 1), (1, 0, 0), [(c, c + 16) for c in range(0, 144, 16)]),
}


def _weights(cout, cin, k, ranges):
    """[cout, cin, kt, kh, kw] float64: step (tap, range r) of output channel co weighs 1 + (len(ranges) tap + r + co) % S,
    S = 252 // steps, so that an interior output stays <= 252"""
    taps = k[0] * k[1] * k[2]
    steps = taps * len(ranges)
    span = 252 // steps
    w = torch.zeros(cout, cin, taps, dtype=torch.float64)
    for co in range(cout):
        for tap in range(taps):
            for r, (lo, hi) in enumerate(ranges):
                w[co, lo:hi, tap] = 1 + (len(ranges) * tap + r + co) % span
    return w.view(cout, cin, *k)


def _run(name, dtype, geom, epilogue, seed=0):
    from dvt_amd import ops
    Cin, Cout, k, pad, ranges = HALVES[name]
    N, T, H, W = geom
    x64 = one_hot_input(N * T * H * W, Cin, ranges, seed=seed)                  # NDHWC rows
    w64 = _weights(Cout, Cin, k, ranges)
    x = x64.to(dtype).cuda()
    K = ops.conv3d_implicit_k(x, geom, Cout, k, (1, 1, 1), pad)
    wp = ops.conv3d_weight_pack(w64.float().cuda(), Cin, K, dtype)
    ref = TF.conv3d(x64.view(N, T, H, W, Cin).permute(0, 4, 1, 2, 3), w64, padding=pad)
    ref = ref.permute(0, 2, 3, 4, 1).reshape(-1, Cout)                          # exact integers
    assert ref.abs().max() <= 256
    kw = {}
    if epilogue:
        g = torch.Generator().manual_seed(seed + 1)
        scale = 2.0 ** torch.randint(-2, 2, (Cout,), generator=g).double()
        shift = torch.randint(-8, 8, (Cout,), generator=g).double()
        res = torch.randint(-16, 16, (ref.shape[0], Cout), generator=g).double()
        ref = torch.relu(ref * scale + shift + res)                           # exact in fp32; one rounding to dtype
        kw = dict(scale=scale.float().cuda(), shift=shift.float().cuda(), residual=res.to(dtype).cuda(), relu=True)
    y = ops.conv2p1d_l1(x, wp, geom, Cout, k, (1, 1, 1), pad, **kw)
    return y, ref.to(dtype), (x, wp, kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["spatial", "temporal"])
@pytest.mark.parametrize("geom", [(2, 5, 9, 11), (1, 3, 56, 56)], ids=["odd", "l1map"])
def test_conv2p1d_l1_exact(device, name, dtype, geom):
    y, ref, _ = _run(name, dtype, geom, epilogue=False)
    assert torch.equal(y.cpu(), ref)
    # interior outputs: every k-step of every tap contributed (the sum of the steps' distinct weights)
    assert int(ref.float().max()) > 100


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["spatial", "temporal"])
def test_conv2p1d_l1_epilogue_exact_and_repeatable(device, name, dtype):
    from dvt_amd import ops
    Cin, Cout, k, pad, _ = HALVES[name]
    geom = (2, 4, 13, 10)
    y, ref, (x, wp, kw) = _run(name, dtype, geom, epilogue=True, seed=3)
    assert torch.equal(y.cpu(), ref)
    y2 = ops.conv2p1d_l1(x, wp, geom, Cout, k, (1, 1, 1), pad, **kw)
    assert torch.equal(y, y2)                                                     # bitwise repeatable
    # the same packed weights and epilogue on dvt_conv3d_implicit: the same exact result
    y3 = ops.conv3d_implicit(x, wp, geom, Cout, k, (1, 1, 1), pad, **kw)
    assert torch.equal(y, y3)


def test_conv2p1d_l1_supported_geometries(device):
    from dvt_amd import ops
    x64 = torch.zeros(2 * 3 * 8 * 8, 64, dtype=torch.bfloat16, device="cuda")
    x144 = torch.zeros(2 * 3 * 8 * 8, 144, dtype=torch.bfloat16, device="cuda")
    g = (2, 3, 8, 8)
    assert ops.conv2p1d_l1_supported(x64, g, 144, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    assert ops.conv2p1d_l1_supported(x144, g, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    assert not ops.conv2p1d_l1_supported(x64, g, 144, (1, 3, 3), (1, 2, 2), (0, 1, 1))       # strided
    assert not ops.conv2p1d_l1_supported(x64, g, 232, (1, 3, 3), (1, 1, 1), (0, 1, 1))       # layer 2
    assert not ops.conv2p1d_l1_supported(x64.float(), g, 144, (1, 3, 3), (1, 1, 1), (0, 1, 1))   # fp32
