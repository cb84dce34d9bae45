"""Every data-movement kernel of csrc/conv.hip -- im2col, col2im, the weight pack / unpack forms, pad3 / unpad3, the
pixel-pair weights and the NCHW -> NHWC layouts -- called directly through ops.* and compared with the index arithmetic of
tests/convdata_ref.py.  No tolerance: a move is the float64 operand rounded once to the output dtype, compared bit for bit
(signed zeros, bf16 / fp16 rounding ties and the largest finite source value are among the operands); a col2im sum has integer
operands bounded so that the largest possible sum is exact in the output dtype (``check_bound``), so torch.equal holds in any
summation order.  One case per col2im kernel uses ordinary random values under the rule of tests/rowwise_ref.py.

Operands are rounded to the kernel's dtype before the reference and the kernel see them.  Outputs ops allocates sit in the
NaN bands of ``guarded``, destinations the caller owns come from ``poisoned`` / ``canaried``; where ld exceeds the columns a
kernel may read (col2im, unpack) the padding columns of the input are NaN, so a read of them shows in the result.
tests/test_conv_data_coverage.py ties every kernel symbol of the built library to a parameter set of this file, and
tests/test_conv_data_cpu.py asserts through the mirrors of convdata_ref that the tables below reach what they name.

What each table is there for (N = 2 throughout):
  IM2COL_GEOMS   C = 5 on 7 x 10, k (3,2) / s (2,1) / p (1,0), ld = K + 10: every geometry parameter asymmetric; 8 x 12 with
                 k 3 / s 2 / p 0: (H + 2p - k) % s != 0, the last rows and columns are never read; 7 x 9 with k 1 / s 2 / p 0:
                 the downsample fork's gather on an odd map.
  IM2COL_FALLBACKS  calls one condition short of the stem or the vector kernel, which must run im2col_kernel.
  STEM_GEOMS     9 x 12, k 7: ld = 152 (the last 8-column chunk straddles K = 147), ld = 160 (a whole zero chunk), and
                 stride (2,1) / pad (3,2).
  VEC_WIDTHS     C = 8 and 16 on 6 x 9, k (3,2) / s (1,2) / p (0,1), ld == K.
  C2I_VEC / C2I_SCALAR / C2I_NCHW   see the comments on the tables.
  PACK_GROUP_CASES  the branches of weight_pack_group_kernel beyond tests/test_gpu_cnn.py's two-transposes test.
  GRID_CAP       per streaming kernel, the smallest call whose item count is 8 x CUs x 256 plus a ragged remainder: the
                 grid-stride loop makes a second, partial trip."""
import ctypes as C_

import pytest
import torch

from tests import convdata_ref as V
from tests import rowwise_ref as R
from tests.gemm_exact import canaried, canaries_intact, check_bound
from tests.guards import guarded, poisoned

pytestmark = pytest.mark.gpu

N = 2
DT = V.NAMES
PAIR_IDS7 = [V.pair_id(p) for p in V.PAIRS7]
PAIR_IDS6 = [V.pair_id(p) for p in V.PAIRS6]
NAN = float("nan")

# (C, H, W, k, stride, pad, ld - K)
IM2COL_GEOMS = [(5, 7, 10, (3, 2), (2, 1), (1, 0), 10), (5, 8, 12, 3, 2, 0, 0), (5, 7, 9, 1, 2, 0, 3)]
# name -> (x dtype, out dtype, nchw, C, H, W, k, stride, pad, ld - K, x one element past a 16-byte boundary)
IM2COL_FALLBACKS = {
    "nchw3k7-ld147": ("fp32", "bf16", True, 3, 9, 12, 7, 2, 3, 0, False),
    "nhwc8-ldpad8": ("bf16", "bf16", False, 8, 6, 9, (3, 2), (1, 2), (0, 1), 8, False),
    "nhwc8-misaligned": ("bf16", "bf16", False, 8, 6, 9, (3, 2), (1, 2), (0, 1), 0, True),
    "nhwc8-converting": ("fp32", "fp16", False, 8, 6, 9, (3, 2), (1, 2), (0, 1), 0, False),
}
# (H, W, stride, pad, ld)
STEM_GEOMS = [(9, 12, 2, 3, 152), (9, 12, 2, 3, 160), (9, 12, (2, 1), (3, 2), 152)]
VEC_WIDTHS = [8, 16]
VEC_GEOM = (6, 9, (3, 2), (1, 2), (0, 1))
# name -> (C, H, W, k, stride, pad, ld - K, add: None | "full" | "compact")
C2I_VEC = {
    "c8-k3s2p1": (8, 7, 10, 3, 2, 1, 0, None),
    "c16-k3s2p1": (16, 7, 10, 3, 2, 1, 0, None),
    "c8-k32s12": (8, 7, 10, (3, 2), (1, 2), (1, 0), 0, None),
    "c16-k32s12": (16, 7, 10, (3, 2), (1, 2), (1, 0), 0, None),
    "c8-k1s2p0": (8, 7, 9, 1, 2, 0, 0, None),
    "c8-ldpad8": (8, 7, 10, 3, 2, 1, 8, None),
    "c8-add-full": (8, 7, 10, 3, 2, 1, 0, "full"),
    "c16-add-compact": (16, 7, 9, 3, 2, 1, 8, "compact"),          # odd H and W: the compact map is 4 x 5
}
# name -> (C, H, W, k, stride, pad, ld - K, dcol one element past a 16-byte boundary)
C2I_SCALAR = {
    "c5": (5, 7, 10, (3, 2), (2, 1), (1, 0), 3, False),
    "c8-misaligned": (8, 7, 10, 3, 2, 1, 0, True),
    "kw7-sw1": (5, 6, 11, (2, 7), 1, (0, 3), 5, False),             # seven taps of a row: a full batch of four and three
    "kw7-sw2": (5, 6, 11, (2, 7), (1, 2), (0, 3), 0, False),        # four or three taps of a row in one batch
    "edges": (3, 8, 5, (5, 1), (2, 1), (1, 0), 1, False),           # Ho = 3: ho >= Ho at h = 7 (ki 0), hh < 0 at h = 0
}
C2I_NCHW = (3, 9, 12, 7, 2, 3, 152)                                  # C, H, W, k, stride, pad, ld
# name -> [(cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind, cls, src one float past a 16-byte boundary)]
PACK_GROUP_CASES = {
    "kind2-s22": [(5, 6, 3, 3, 8, 8, 0, 2, (2, 2, rh, rw), False) for rh in (0, 1) for rw in (0, 1)],
    "kind2-s21": [(6, 5, 3, 2, 6, 7, 0, 2, (2, 1, rh, 0), False) for rh in (0, 1)],
    "elems-rowlen": [(3, 1030, 3, 3, 3, 1032, 9296, 0, None, False)],
    "elems-ld": [(2, 8, 1, 1, 2, 8, 32776, 0, None, False)],
    "misaligned-src": [(5, 4, 3, 3, 8, 8, 80, 0, None, True), (5, 4, 3, 3, 8, 8, 0, 1, None, True)],
    "scalar-store-cin": [(6, 5, 3, 1, 8, 6, 24, 0, None, False)],
    "scalar-store-cout": [(5, 8, 3, 1, 6, 8, 0, 1, None, False)],
    "rows-r1": [(3, 8, 3, 3, 3, 8, 2048, 0, None, False)],
    "rows-r3-ragged": [(5, 8, 3, 3, 7, 8, 640, 0, None, False)],   # R = 3, cout_p = 7: the last workgroup has one row
}
NHWC_PAD8 = ([1, 3, 8], 3, 5)
NHWC_PAIR4 = ([1, 3, 4], 3, 6)
PAIR_GEOMS = [(7, 3, 4), (7, 2, 4), (6, 0, 3)]                       # (kw, pw, kwp): off = 1, 0, 0
PAIR_CIN = [1, 3, 4]
GRID_CAP = ["im2col", "im2col_stem", "im2col_vec", "col2im_nhwc", "col2im_scalar", "col2im_nchw", "weight_pack",
            "weight_pack_dgrad", "weight_unpack", "weight_unpack_t", "pad3", "unpad3", "nhwc_pad8", "nhwc_pair4",
            "weight_pairs", "weight_pairs_bwd"]
RAGGED = 77


@pytest.fixture(scope="module")
def dvt(device):
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _cu_count(dvt):
    """the compute-unit count the library sizes its grids by"""
    n = C_.c_int(0)
    dvt._lib.check(dvt._lib.load().dvt_device_info(C_.byref(n), None, None, 0), "dvt_device_info")
    assert n.value > 0
    return n.value


def _off_by_one(t, device):
    """t on the device, one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def _dev(t, dtype, device, misaligned=False):
    t = t.to(dtype).contiguous()
    return _off_by_one(t, device) if misaligned else t.to(device)


def _exact(got, ref64, what):
    want = V.rounded_to(ref64, got.dtype)
    assert V.same_bits(got.cpu(), want.reshape(got.shape)), \
        f"{what}: {int((got.cpu().double() != want.reshape(got.shape).double()).sum())} of {got.numel()} elements differ"


def _K(C, k):
    kh, kw = V.pair(k)
    return kh * kw * C


# ---------------------------------------------------------------- im2col
def _im2col_case(ops, device, src, dst, nchw, C, H, W, k, stride, pad, ld, seed, misaligned=False):
    sd, dd = V.DTYPES[src], V.DTYPES[dst]
    x = V.move_values((N, C, H, W) if nchw else (N, H, W, C), sd, seed)
    with guarded(ops):
        out = ops.im2col(_dev(x, sd, device, misaligned), nchw, N, C, H, W, k, stride, pad, ld, dd)
    _exact(out, V.im2col(x, nchw, N, C, H, W, k, stride, pad, ld), f"im2col {src}->{dst} nchw={nchw} C={C} {H}x{W} k={k} ld={ld}")


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("pair", V.PAIRS7, ids=PAIR_IDS7)
def test_im2col(dvt, device, pair, layout):
    """im2col_kernel<S, D, NCHW>: the three geometries of IM2COL_GEOMS"""
    for i, (C, H, W, k, s, p, extra) in enumerate(IM2COL_GEOMS):
        _im2col_case(dvt.ops, device, pair[0], pair[1], layout == "nchw", C, H, W, k, s, p, _K(C, k) + extra, 100 + i)


@pytest.mark.parametrize("case", list(IM2COL_FALLBACKS))
def test_im2col_fallbacks(dvt, device, case):
    """one condition short of the stem / vector kernel: the element-per-thread kernel must take the call"""
    src, dst, nchw, C, H, W, k, s, p, extra, mis = IM2COL_FALLBACKS[case]
    _im2col_case(dvt.ops, device, src, dst, nchw, C, H, W, k, s, p, _K(C, k) + extra, 110, misaligned=mis)


@pytest.mark.parametrize("pair", V.PAIRS7, ids=PAIR_IDS7)
def test_im2col_stem(dvt, device, pair):
    """im2col_nchw_stem_kernel<S, D, 3, 7, 7>"""
    for i, (H, W, s, p, ld) in enumerate(STEM_GEOMS):
        _im2col_case(dvt.ops, device, pair[0], pair[1], True, 3, H, W, 7, s, p, ld, 120 + i)


@pytest.mark.parametrize("C", VEC_WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_im2col_vec(dvt, device, name, C):
    """im2col_nhwc_vec_kernel<T>"""
    H, W, k, s, p = VEC_GEOM
    _im2col_case(dvt.ops, device, name, name, False, C, H, W, k, s, p, _K(C, k), 130 + C)


# ---------------------------------------------------------------- col2im
def _dcol(rows, K, ld, bound, seed):
    """integer columns with NaN in the K padding"""
    d = torch.full((rows, ld), NAN, dtype=torch.float64)
    d[:, :K] = V.int_values((rows, K), bound, seed)
    return d


def _add_operand(add, C, H, W, bound, seed):
    if add is None:
        return None, 0
    if add == "full":
        return V.int_values((N * H * W, C), bound, seed), 0
    return V.int_values((N * -(-H // 2) * -(-W // 2), C), bound, seed), 2


def _col2im_case(ops, device, name, C, H, W, k, s, p, extra, add=None, misaligned=False, seed=0):
    dtype = V.DTYPES[name]
    Ho, Wo = V.out_hw(H, W, k, s, p)
    K = _K(C, k)
    bound = V.c2i_bound(k, s, add is not None, dtype)
    d = _dcol(N * Ho * Wo, K, K + extra, bound, seed)
    a, a_stride = _add_operand(add, C, H, W, bound, seed + 1)
    ref = V.col2im(d, N, C, H, W, k, s, p, add=a, add_stride=a_stride)
    check_bound(ref, dtype)
    with guarded(ops):
        dx = ops.col2im(_dev(d, dtype, device, misaligned), N, C, H, W, k, s, p,
                        add=None if a is None else _dev(a, dtype, device), add_stride=a_stride)
    assert torch.equal(dx.cpu(), ref.to(dtype)), f"col2im {name} C={C} {H}x{W} k={k} s={s} p={p} add={add}"


@pytest.mark.parametrize("case", list(C2I_VEC))
@pytest.mark.parametrize("name", DT)
def test_col2im_nhwc(dvt, device, name, case):
    """col2im_nhwc_kernel<T>"""
    C, H, W, k, s, p, extra, add = C2I_VEC[case]
    _col2im_case(dvt.ops, device, name, C, H, W, k, s, p, extra, add=add, seed=200)


@pytest.mark.parametrize("case", list(C2I_SCALAR))
@pytest.mark.parametrize("name", DT)
def test_col2im_scalar(dvt, device, name, case):
    """col2im_scalar_kernel<T, T, false>"""
    C, H, W, k, s, p, extra, mis = C2I_SCALAR[case]
    _col2im_case(dvt.ops, device, name, C, H, W, k, s, p, extra, misaligned=mis, seed=210)


@pytest.mark.parametrize("name", DT)
def test_col2im_second_path_needs_the_vector_route(dvt, device, name):
    """add with C % 8 != 0 is refused with the unsupported code, before any launch"""
    dtype = V.DTYPES[name]
    C, H, W = 5, 7, 10
    Ho, Wo = V.out_hw(H, W, 3, 2, 1)
    d = torch.zeros(N * Ho * Wo, 9 * C, dtype=dtype, device=device)
    a = torch.zeros(N * H * W, C, dtype=dtype, device=device)
    with pytest.raises(RuntimeError, match=r"status -2"):
        dvt.ops.col2im(d, N, C, H, W, 3, 2, 1, add=a)


@pytest.mark.parametrize("pair", V.PAIRS7, ids=PAIR_IDS7)
def test_col2im_nchw(dvt, device, pair):
    """col2im_scalar_kernel<S, D, true>: the stem's input gradient"""
    sd, dd = V.DTYPES[pair[0]], V.DTYPES[pair[1]]
    C, H, W, k, s, p, ld = C2I_NCHW
    Ho, Wo = V.out_hw(H, W, k, s, p)
    d = _dcol(N * Ho * Wo, _K(C, k), ld, V.c2i_bound(k, s, False, sd, dd), 220)
    ref = V.col2im(d, N, C, H, W, k, s, p, nchw=True)
    check_bound(ref, dd)
    with guarded(dvt.ops):
        dx = dvt.ops.col2im_nchw(_dev(d, sd, device), N, C, H, W, k, s, p, dd)
    assert torch.equal(dx.cpu(), ref.to(dd)), f"col2im_nchw {pair}"


@pytest.mark.parametrize("route", ["nhwc", "scalar", "nchw"])
@pytest.mark.parametrize("name", DT)
def test_col2im_random_values(dvt, device, name, route):
    """ordinary values: each pixel's sum within the budget of tests/rowwise_ref.py around the float64 scatter-add"""
    dtype, ops = V.DTYPES[name], dvt.ops
    C, H, W, k, s, p = {"nhwc": (16, 7, 10, 3, 2, 1), "scalar": (5, 6, 11, (2, 7), 1, (0, 3)), "nchw": C2I_NCHW[:6]}[route]
    Ho, Wo = V.out_hw(H, W, k, s, p)
    K = _K(C, k)
    ld = K + 8 if route != "nchw" else C2I_NCHW[6]
    g = torch.Generator().manual_seed(230)
    d = torch.full((N * Ho * Wo, ld), NAN, dtype=torch.float64)
    d[:, :K] = torch.randn(N * Ho * Wo, K, generator=g, dtype=torch.float64).to(dtype).double()
    dz = torch.nan_to_num(d, nan=0.0)                                 # the statement never reads the padding
    ref = V.col2im(dz, N, C, H, W, k, s, p, nchw=route == "nchw")
    chain = V.col2im(dz.float(), N, C, H, W, k, s, p, nchw=route == "nchw")
    mag = float(dz.abs().max())
    with guarded(ops):
        if route == "nchw":
            dx = ops.col2im_nchw(_dev(d, dtype, device), N, C, H, W, k, s, p, dtype)
        else:
            dx = ops.col2im(_dev(d, dtype, device), N, C, H, W, k, s, p)
    R.assert_close(dx.cpu(), ref, chain, mag, f"col2im random {name} {route}")


# ---------------------------------------------------------------- weight forms
W_SHAPE = (5, 3, 3, 2)                                               # Cout, Cin, kh, kw


@pytest.mark.parametrize("extra", [0, 6])
@pytest.mark.parametrize("name", DT)
def test_weight_pack(dvt, device, name, extra):
    """weight_pack_kernel<D>"""
    w = V.move_values(W_SHAPE, torch.float32, 300)
    ld = W_SHAPE[1] * W_SHAPE[2] * W_SHAPE[3] + extra
    with guarded(dvt.ops):
        out = dvt.ops.conv_weight_pack(_dev(w, torch.float32, device), ld, V.DTYPES[name])
    _exact(out, V.weight_pack(w, ld), f"weight_pack {name} ld={ld}")


@pytest.mark.parametrize("name", DT)
def test_weight_pack_dgrad(dvt, device, name):
    """weight_pack_dgrad_kernel<D>"""
    w = V.move_values(W_SHAPE, torch.float32, 301)
    with guarded(dvt.ops):
        out = dvt.ops.conv_weight_pack_dgrad(_dev(w, torch.float32, device), V.DTYPES[name])
    _exact(out, V.weight_pack_dgrad(w), f"weight_pack_dgrad {name}")


def _into(device, shape, accumulate, run, ref64, what):
    """run(out, accumulate) into a poisoned destination that holds 3.0: the result is ref (+ 3.0 when accumulate)"""
    out, chk = poisoned(shape, torch.float32, device, fill=3.0)
    run(out, accumulate)
    chk()
    want = ref64.reshape(shape) + (3.0 if accumulate else 0.0)
    assert torch.equal(out.cpu(), want.float()), what


@pytest.mark.parametrize("accumulate", [False, True])
def test_weight_unpack(dvt, device, accumulate):
    """weight_unpack_kernel: ld = K and K + 6 (NaN in the padding columns)"""
    Cout, Cin, kh, kw = W_SHAPE
    K = Cin * kh * kw
    for extra in (0, 6):
        g = torch.full((Cout, K + extra), NAN, dtype=torch.float64)
        g[:, :K] = V.int_values((Cout, K), 1000, 310)
        gd = _dev(g, torch.float32, device)
        _into(device, W_SHAPE, accumulate, lambda out, acc: dvt.ops.conv_weight_unpack_grad(gd, W_SHAPE, out=out, accumulate=acc),
              V.weight_unpack(g, W_SHAPE), f"weight_unpack ld=K+{extra} accumulate={accumulate}")
    with guarded(dvt.ops):
        out = dvt.ops.conv_weight_unpack_grad(gd, W_SHAPE)
    assert torch.equal(out.cpu(), V.weight_unpack(g, W_SHAPE).float())


@pytest.mark.parametrize("accumulate", [False, True])
def test_weight_unpack_t(dvt, device, accumulate):
    """weight_unpack_t_kernel"""
    Cout, Cin, kh, kw = W_SHAPE
    gt = V.int_values((Cin * kh * kw, Cout), 1000, 311)
    gd = _dev(gt, torch.float32, device)
    _into(device, W_SHAPE, accumulate, lambda out, acc: dvt.ops.conv_weight_unpack_grad_t(gd, W_SHAPE, out=out, accumulate=acc),
          V.weight_unpack_t(gt, W_SHAPE), f"weight_unpack_t accumulate={accumulate}")


@pytest.mark.parametrize("case", ["3x5x6-to-4x8x6", "identity"])
def test_pad3(dvt, device, case):
    """pad3_kernel"""
    A, B, K = 3, 5, 6
    Ap, Bp = (4, 8) if case != "identity" else (A, B)
    src = V.move_values((A, B, K), torch.float32, 320)
    with guarded(dvt.ops):
        out = dvt.ops.pad3_f32(_dev(src, torch.float32, device), A, B, K, Ap, Bp)
    _exact(out, V.pad3(src, Ap, Bp), f"pad3 {case}")


@pytest.mark.parametrize("accumulate", [False, True])
def test_unpad3(dvt, device, accumulate):
    """unpad3_kernel: the slice [:3, :5] of [4, 8, 6]; what lies outside the slice is NaN"""
    A, B, K, Ap, Bp = 3, 5, 6, 4, 8
    src = torch.full((Ap, Bp, K), NAN, dtype=torch.float64)
    src[:A, :B] = V.int_values((A, B, K), 1000, 321)
    sd = _dev(src, torch.float32, device)
    _into(device, (A, B, K), accumulate, lambda out, acc: dvt.ops.unpad3_f32(sd, A, B, K, Bp, out=out, accumulate=acc),
          V.unpad3(src, A, B), f"unpad3 accumulate={accumulate}")
    if not accumulate:
        with guarded(dvt.ops):
            out = dvt.ops.unpad3_f32(sd, A, B, K, Bp)
        assert torch.equal(out.cpu(), V.unpad3(src, A, B).float())


@pytest.mark.parametrize("geom", PAIR_GEOMS, ids=[f"kw{a}pw{b}kwp{c}" for a, b, c in PAIR_GEOMS])
@pytest.mark.parametrize("Cin", PAIR_CIN)
def test_weight_pairs(dvt, device, Cin, geom):
    """conv_weight_pairs_kernel"""
    kw, pw, kwp = geom
    Cout, kh = 5, 3
    w = V.move_values((Cout, Cin, kh, kw), torch.float32, 330 + Cin)
    with guarded(dvt.ops):
        wp = dvt.ops.conv_weight_pairs(_dev(w, torch.float32, device), Cout, Cin, kh, kw, pw, kwp)
    _exact(wp, V.weight_pairs(w, pw, kwp), f"weight_pairs Cin={Cin} {geom}")


@pytest.mark.parametrize("geom", PAIR_GEOMS, ids=[f"kw{a}pw{b}kwp{c}" for a, b, c in PAIR_GEOMS])
@pytest.mark.parametrize("Cin", PAIR_CIN)
@pytest.mark.parametrize("accumulate", [False, True])
def test_weight_pairs_bwd(dvt, device, accumulate, Cin, geom):
    """conv_weight_pairs_bwd_kernel: the positions of dwp the adjoint never reads (c >= Cin, kj outside the kernel) are NaN"""
    kw, pw, kwp = geom
    Cout, kh = 5, 3
    vals = V.int_values((Cout, 8, kh, kwp), 1000, 340 + Cin)
    read = V.weight_pairs(torch.ones(Cout, Cin, kh, kw, dtype=torch.float64), pw, kwp) > 0
    dwp = torch.where(read, vals, torch.full_like(vals, NAN))
    dd = _dev(dwp, torch.float32, device)
    _into(device, (Cout, Cin, kh, kw), accumulate,
          lambda out, acc: dvt.ops.conv_weight_pairs_bwd(dd, Cout, Cin, kh, kw, pw, kwp, out=out, accumulate=acc),
          V.weight_pairs_bwd(vals, Cin, kw, pw), f"weight_pairs_bwd Cin={Cin} {geom} accumulate={accumulate}")


# ---------------------------------------------------------------- the grouped pack
def _pack_entries(device, dtype, rows, seed):
    """[(ops entry, canary buffer, destination shape, float64 reference)] of rows of PACK_GROUP_CASES' form"""
    out = []
    for i, (co, ci, kh, kw, cop, cip, ld, kind, cls, mis) in enumerate(rows):
        w = V.move_values((co, ci, kh, kw), torch.float32, seed + i)
        ref = V.weight_pack_group(w, kind, cop, cip, ld, cls)
        buf, view = canaried(ref.shape[0], ref.shape[1], dtype, device, pad=0, spare=1)
        src = _dev(w.reshape(co, ci, kh * kw), torch.float32, device, mis)
        entry = (src, view, co, ci, kh, kw, cop, cip, ld, kind) + ((cls,) if kind == 2 else ())
        out.append((entry, buf, ref))
    return out


def _check_packed(packed, what):
    for i, (entry, buf, ref) in enumerate(packed):
        assert canaries_intact(buf, *ref.shape) == 0, f"{what} entry {i}: wrote past the destination"
        _exact(entry[1], ref, f"{what} entry {i} {entry[2:]}")


@pytest.mark.parametrize("case", list(PACK_GROUP_CASES))
@pytest.mark.parametrize("name", DT)
def test_pack_group(dvt, device, name, case):
    """weight_pack_group_kernel: the branches PACK_GROUP_CASES names, each judged against the per-tap statement"""
    packed = _pack_entries(device, V.DTYPES[name], PACK_GROUP_CASES[case], 400)
    dvt.ops.conv_weight_pack_group([p[0] for p in packed])
    _check_packed(packed, f"pack_group {name} {case}")


@pytest.mark.parametrize("name", DT)
def test_pack_group_two_launches_and_none(dvt, device, name):
    """41 entries (the 41st in a launch of its own), of all three kinds; count == 0 launches nothing"""
    kinds = [(4, 3, 3, 2, 5, 4, 40, 0, None, False), (4, 3, 3, 2, 5, 4, 0, 1, None, False), (4, 3, 3, 2, 5, 4, 0, 2, (2, 1, 1, 0), False)]
    packed = _pack_entries(device, V.DTYPES[name], [kinds[i % 3] for i in range(V.PACK_GROUP + 1)], 450)
    dvt.ops.conv_weight_pack_group([p[0] for p in packed])
    _check_packed(packed, f"pack_group {name} 41 entries")
    dvt.ops.conv_weight_pack_group([])
    assert dvt._lib.load().dvt_conv_weight_pack_group(None, 0, None) == 0


# ---------------------------------------------------------------- layouts
def _layout_case(ops, device, pair, C, H, W, cpad, seed):
    sd, dd = V.DTYPES[pair[0]], V.DTYPES[pair[1]]
    x = V.move_values((N, C, H, W), sd, seed)
    with guarded(ops):
        y = ops.nchw_to_nhwc_pad(_dev(x, sd, device), dd, cpad)
    _exact(y, V.nhwc_pad8(x) if cpad == 8 else V.nhwc_pair4(x), f"nchw_to_nhwc_pad {pair} C={C} cpad={cpad}")


@pytest.mark.parametrize("C", NHWC_PAD8[0])
@pytest.mark.parametrize("pair", V.PAIRS6, ids=PAIR_IDS6)
def test_nhwc_pad8(dvt, device, pair, C):
    """nchw_to_nhwc_pad8_kernel<S, D>"""
    _layout_case(dvt.ops, device, pair, C, NHWC_PAD8[1], NHWC_PAD8[2], 8, 500 + C)


@pytest.mark.parametrize("C", NHWC_PAIR4[0])
@pytest.mark.parametrize("pair", V.PAIRS6, ids=PAIR_IDS6)
def test_nhwc_pair4(dvt, device, pair, C):
    """nchw_to_nhwc_pair4_kernel<S, D>"""
    _layout_case(dvt.ops, device, pair, C, NHWC_PAIR4[1], NHWC_PAIR4[2], 4, 510 + C)


def test_nhwc_pad_rejects(dvt, device):
    """an fp32 output, an odd W with Cpad = 4, and C > Cpad are refused before any launch"""
    x = torch.zeros(N, 3, 3, 6, device=device)
    for bad in (lambda: dvt.ops.nchw_to_nhwc_pad(x, torch.float32, 8), lambda: dvt.ops.nchw_to_nhwc_pad(x, torch.float32, 4),
                lambda: dvt.ops.nchw_to_nhwc_pad(torch.zeros(N, 3, 3, 5, device=device), torch.bfloat16, 4),
                lambda: dvt.ops.nchw_to_nhwc_pad(torch.zeros(N, 5, 3, 6, device=device), torch.bfloat16, 4),
                lambda: dvt.ops.nchw_to_nhwc_pad(torch.zeros(N, 9, 3, 6, device=device), torch.bfloat16, 8)):
        with pytest.raises(RuntimeError, match=r"status -1"):
            bad()


# ---------------------------------------------------------------- grid cap and empty batch
def grid_cap_call(family, cap):
    """(item count of the kernel's grid-stride loop, the call's shape parameters) of the GRID_CAP case of ``family``: the
    fewest channels with which the items pass ``cap`` by a ragged remainder"""
    want = cap + RAGGED
    if family == "im2col":                     # items = rows * ld; C = 1, one image row, k (1,2), p (0,1): Wo = W + 1, ld = 2
        W = -(-want // 2) - 1
        return (W + 1) * 2, dict(W=W)
    if family == "im2col_stem":                # items = rows * ld / 8; one image row of width W, k 7 / s 1 / p 3, ld 152: 19 chunks
        W = -(-want // 19)
        return W * 19, dict(W=W)
    if family == "im2col_vec":                 # items = rows * kh * kw * C / 8; C = 8, k (1,2), p (0,1)
        W = -(-want // 2) - 1
        return (W + 1) * 2, dict(W=W)
    if family == "col2im_nhwc":                # items = N * H * W * C / 8
        return want, dict(W=want)
    if family in ("col2im_scalar", "col2im_nchw"):   # items = N * H * W * C, C = 1
        return want, dict(W=want)
    if family in ("weight_pack", "weight_pack_dgrad", "weight_unpack", "weight_unpack_t"):   # items = Cout * Cin * kh * kw
        Cout = -(-want // 6)
        return Cout * 6, dict(Cout=Cout)
    if family in ("pad3", "unpad3"):           # items = A * B * K of the destination
        A = -(-want // 6)
        return A * 6, dict(A=A)
    if family == "nhwc_pad8":                  # items = N * H * W
        return want, dict(W=want)
    if family == "nhwc_pair4":                 # items = N * H * W / 2
        return want, dict(W=2 * want)
    Cout = -(-want // 24)                      # weight_pairs: Cout * 8 * kh * kwp (1, 3); its adjoint: Cout * Cin * kh * kw (4, 3, 2)
    return Cout * 24, dict(Cout=Cout)


@pytest.mark.parametrize("family", GRID_CAP)
def test_grid_cap(dvt, device, family):
    """more items than the capped grid covers in one trip, by a ragged remainder (bf16 / fp32 as the kernel takes)"""
    ops = dvt.ops
    cap = V.grid_cap(_cu_count(dvt))
    items, q = grid_cap_call(family, cap)
    assert cap < items < cap + 256, (family, items, cap)
    bf, f32 = torch.bfloat16, torch.float32
    if family in ("im2col", "im2col_vec"):
        C = 1 if family == "im2col" else 8
        x = V.move_values((1, 1, q["W"], C), bf, 600)
        with guarded(ops):
            out = ops.im2col(_dev(x, bf, device), False, 1, C, 1, q["W"], (1, 2), 1, (0, 1), 2 * C, bf)
        _exact(out, V.im2col(x, False, 1, C, 1, q["W"], (1, 2), 1, (0, 1), 2 * C), family)
    elif family == "im2col_stem":
        x = V.move_values((1, 3, 1, q["W"]), bf, 601)
        with guarded(ops):
            out = ops.im2col(_dev(x, bf, device), True, 1, 3, 1, q["W"], 7, 1, 3, 152, bf)
        _exact(out, V.im2col(x, True, 1, 3, 1, q["W"], 7, 1, 3, 152), family)
    elif family in ("col2im_nhwc", "col2im_scalar", "col2im_nchw"):
        C = 8 if family == "col2im_nhwc" else 1
        W = q["W"]                                                                   # k (1,2), p (0,1): Wo = W + 1
        d = V.int_values((W + 1, 2 * C), V.c2i_bound((1, 2), 1, False, bf), 602)
        ref = V.col2im(d, 1, C, 1, W, (1, 2), 1, (0, 1), nchw=family == "col2im_nchw")
        check_bound(ref, bf)
        with guarded(ops):
            if family == "col2im_nchw":
                dx = ops.col2im_nchw(_dev(d, bf, device), 1, C, 1, W, (1, 2), 1, (0, 1), bf)
            else:
                dx = ops.col2im(_dev(d, bf, device), 1, C, 1, W, (1, 2), 1, (0, 1))
        assert torch.equal(dx.cpu(), ref.to(bf)), family
    elif family in ("weight_pack", "weight_pack_dgrad"):
        w = V.move_values((q["Cout"], 1, 3, 2), f32, 603)
        with guarded(ops):
            out = ops.conv_weight_pack(_dev(w, f32, device), 6, bf) if family == "weight_pack" else \
                ops.conv_weight_pack_dgrad(_dev(w, f32, device), bf)
        _exact(out, V.weight_pack(w, 6) if family == "weight_pack" else V.weight_pack_dgrad(w), family)
    elif family in ("weight_unpack", "weight_unpack_t"):
        shape = (q["Cout"], 1, 3, 2)
        g = V.move_values((q["Cout"], 6) if family == "weight_unpack" else (6, q["Cout"]), f32, 604)
        with guarded(ops):
            out = (ops.conv_weight_unpack_grad if family == "weight_unpack" else ops.conv_weight_unpack_grad_t)(_dev(g, f32, device), shape)
        _exact(out, V.weight_unpack(g, shape) if family == "weight_unpack" else V.weight_unpack_t(g, shape), family)
    elif family == "pad3":
        src = V.move_values((q["A"] - 1, 2, 2), f32, 605)
        with guarded(ops):
            out = ops.pad3_f32(_dev(src, f32, device), q["A"] - 1, 2, 2, q["A"], 3)
        _exact(out, V.pad3(src, q["A"], 3), family)
    elif family == "unpad3":
        src = V.move_values((q["A"], 4, 2), f32, 606)
        with guarded(ops):
            out = ops.unpad3_f32(_dev(src, f32, device), q["A"], 3, 2, 4)
        _exact(out, V.unpad3(src, q["A"], 3), family)
    elif family in ("nhwc_pad8", "nhwc_pair4"):
        x = V.move_values((1, 1, 1, q["W"]), bf, 607)
        with guarded(ops):
            y = ops.nchw_to_nhwc_pad(_dev(x, bf, device), bf, 8 if family == "nhwc_pad8" else 4)
        _exact(y, V.nhwc_pad8(x) if family == "nhwc_pad8" else V.nhwc_pair4(x), family)
    elif family == "weight_pairs":
        w = V.move_values((q["Cout"], 1, 1, 5), f32, 608)
        with guarded(ops):
            wp = ops.conv_weight_pairs(_dev(w, f32, device), q["Cout"], 1, 1, 5, 3, 3)
        _exact(wp, V.weight_pairs(w, 3, 3), family)
    else:
        assert family == "weight_pairs_bwd"
        dwp = V.move_values((q["Cout"], 8, 3, 1), f32, 609)
        with guarded(ops):
            dw = ops.conv_weight_pairs_bwd(_dev(dwp, f32, device), q["Cout"], 4, 3, 2, 0, 1)
        _exact(dw, V.weight_pairs_bwd(dwp, 4, 2, 0), family)


def test_empty_batch_returns_ok_and_writes_nothing(dvt, device):
    """N == 0: each entry point with the early return answers OK and leaves a poisoned destination as it was"""
    lib = dvt._lib.load()
    bf = torch.bfloat16
    src = torch.zeros(64, dtype=bf, device=device)
    dst, chk = poisoned((64,), bf, device)
    code = dvt._lib.BF16
    assert lib.dvt_im2col(src.data_ptr(), code, 0, dst.data_ptr(), code, 0, 8, 7, 10, 3, 3, 2, 2, 1, 1, 72, None) == 0
    assert lib.dvt_col2im(src.data_ptr(), dst.data_ptr(), 0, 8, 7, 10, 3, 3, 2, 2, 1, 1, 72, None, 0, code, None) == 0
    assert lib.dvt_col2im_nchw(src.data_ptr(), code, dst.data_ptr(), code, 0, 3, 9, 12, 7, 7, 2, 2, 3, 3, 152, None) == 0
    assert lib.dvt_nchw_to_nhwc_pad(src.data_ptr(), code, dst.data_ptr(), code, 0, 3, 3, 6, 8, None) == 0
    assert lib.dvt_nchw_to_nhwc_pad(src.data_ptr(), code, dst.data_ptr(), code, 0, 3, 3, 6, 4, None) == 0
    torch.cuda.synchronize()
    chk()
    assert bool(torch.isnan(dst).all())
