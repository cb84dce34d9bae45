"""CPU checks of tests/convdata_ref.py and of the tables of tests/test_gpu_conv_data.py: the statements are anchored on
torch's own unfold / fold / conv2d (float64), the operands of the GPU cases expose every index slip the statements can
apply to themselves (``fault=``), the shape tables reach the kernels and branches they name (through the dispatch mirrors),
and dvt_col2im / dvt_col2im_nchw refuse the arguments dvt_im2col refuses (before any launch: N = 0 throughout)."""
import itertools

import pytest
import torch
import torch.nn.functional as TF

from tests import convdata_ref as V
from tests import test_gpu_conv_data as T

F64 = torch.float64


def _ints(shape, seed, bound=9):
    return V.int_values(shape, bound, seed)


# ---------------------------------------------------------------- the statements are anchored outside themselves
GEOMS = [(5, 7, 10, (3, 2), (2, 1), (1, 0)), (5, 8, 12, 3, 2, 0), (5, 7, 9, 1, 2, 0), (3, 9, 12, 7, 2, 3), (3, 9, 12, 7, (2, 1), (3, 2)),
         (8, 6, 9, (3, 2), (1, 2), (0, 1)), (5, 6, 11, (2, 7), (1, 2), (0, 3)), (3, 8, 5, (5, 1), (2, 1), (1, 0))]


def _cols_from_unfold(u, N, C, k):
    """unfold's [N, C*kh*kw, L] with (c, ki, kj) column order -> [N*L, (ki, kj, c)]"""
    kh, kw = V.pair(k)
    L = u.shape[2]
    return u.reshape(N, C, kh, kw, L).permute(0, 4, 2, 3, 1).reshape(N * L, kh * kw * C)


def _cols_to_fold(d, N, C, k):
    kh, kw = V.pair(k)
    L = d.shape[0] // N
    return d.reshape(N, L, kh, kw, C).permute(0, 4, 2, 3, 1).reshape(N, C * kh * kw, L)


@pytest.mark.parametrize("geom", GEOMS, ids=[str(i) for i in range(len(GEOMS))])
def test_im2col_is_unfold_and_col2im_is_fold(geom):
    C, H, W, k, s, p = geom
    N = 2
    K = V.pair(k)[0] * V.pair(k)[1] * C
    x = _ints((N, C, H, W), 1)
    want = _cols_from_unfold(TF.unfold(x, V.pair(k), padding=V.pair(p), stride=V.pair(s)), N, C, k)
    for nchw in (True, False):
        xin = x if nchw else x.permute(0, 2, 3, 1).contiguous()
        got = V.im2col(xin, nchw, N, C, H, W, k, s, p, K + 5)
        assert torch.equal(got[:, :K], want) and not got[:, K:].any()
    Ho, Wo = V.out_hw(H, W, k, s, p)
    d = torch.full((N * Ho * Wo, K + 3), float("nan"), dtype=F64)
    d[:, :K] = _ints((N * Ho * Wo, K), 2)
    folded = TF.fold(_cols_to_fold(d[:, :K], N, C, k), (H, W), V.pair(k), padding=V.pair(p), stride=V.pair(s))
    assert torch.equal(V.col2im(d, N, C, H, W, k, s, p, nchw=True), folded)
    assert torch.equal(V.col2im(d, N, C, H, W, k, s, p), folded.permute(0, 2, 3, 1).reshape(N * H * W, C))
    # <im2col(x), d> == <x, col2im(d)>, exactly (integers)
    lhs = (V.im2col(x, True, N, C, H, W, k, s, p, K) * d[:, :K]).sum()
    assert lhs == (x * V.col2im(d, N, C, H, W, k, s, p, nchw=True)).sum() and lhs != 0


def test_col2im_second_path():
    N, C, H, W, k, s, p = 2, 8, 7, 9, 3, 2, 1
    Ho, Wo = V.out_hw(H, W, k, s, p)
    d = _ints((N * Ho * Wo, 9 * C), 3)
    base = V.col2im(d, N, C, H, W, k, s, p)
    full = _ints((N * H * W, C), 4)
    assert torch.equal(V.col2im(d, N, C, H, W, k, s, p, add=full), base + full)
    compact = _ints((N * 4 * 5, C), 5)                    # ceil(7/2) x ceil(9/2)
    spread = torch.zeros(N, H, W, C, dtype=F64)
    for h, w in itertools.product(range(H), range(W)):
        if h % 2 == 0 and w % 2 == 0:
            spread[:, h, w] = compact.reshape(N, 4, 5, C)[:, h // 2, w // 2]
    assert torch.equal(V.col2im(d, N, C, H, W, k, s, p, add=compact, add_stride=2), base + spread.reshape(N * H * W, C))
    # the compact path is the adjoint of the stride-2 subsampling a 1 x 1 / 2 convolution reads
    x = _ints((N, H, W, C), 6)
    assert (x[:, ::2, ::2].reshape(-1, C) * compact).sum() == (x.reshape(-1, C) * spread.reshape(-1, C)).sum()


@pytest.mark.parametrize("k,p", [((3, 2), (1, 0)), ((3, 3), (1, 1)), ((1, 1), (0, 0)), ((2, 5), (1, 3))])
def test_dgrad_pack_is_the_weight_of_the_input_gradient(k, p):
    """used as a stride-1 convolution weight with padding k - 1 - p, the data-gradient form reproduces autograd's dx"""
    Cout, Cin, (kh, kw), (ph, pw) = 5, 3, k, p
    w = _ints((Cout, Cin, kh, kw), 10)
    x = _ints((2, Cin, 7, 10), 11).requires_grad_(True)
    y = TF.conv2d(x, w, padding=(ph, pw))
    dz = _ints(tuple(y.shape), 12)
    dx, = torch.autograd.grad(y, x, dz)
    packed = V.weight_pack_dgrad(w)
    assert packed.shape == (Cin, kh * kw * Cout)
    wd = packed.reshape(Cin, kh, kw, Cout).permute(0, 3, 1, 2)
    assert torch.equal(TF.conv2d(dz, wd, padding=(kh - 1 - ph, kw - 1 - pw)), dx)


def test_forward_pack_is_the_gemm_operand_of_the_convolution():
    """im2col(x) @ pack(w)^T is conv2d, so the two statements agree on the column order"""
    N, Cin, Cout, H, W, k, s, p = 2, 3, 5, 7, 10, (3, 2), (2, 1), (1, 0)
    x, w = _ints((N, Cin, H, W), 13), _ints((Cout, Cin, 3, 2), 14)
    K = 6 * Cin
    y = V.im2col(x, True, N, Cin, H, W, k, s, p, K + 2) @ V.weight_pack(w, K + 2).t()
    Ho, Wo = V.out_hw(H, W, k, s, p)
    assert torch.equal(y.reshape(N, Ho, Wo, Cout).permute(0, 3, 1, 2), TF.conv2d(x, w, stride=s, padding=p))


def test_round_trips_are_the_identity():
    w = _ints((5, 3, 3, 2), 20)
    assert torch.equal(V.weight_unpack(V.weight_pack(w, 18 + 6), tuple(w.shape)), w)
    assert torch.equal(V.weight_unpack_t(V.weight_pack(w, 18).t().contiguous(), tuple(w.shape)), w)
    src = _ints((3, 5, 6), 21)
    assert torch.equal(V.unpad3(V.pad3(src, 4, 8), 3, 5), src) and V.pad3(src, 4, 8).sum() == src.sum()
    assert torch.equal(V.pad3(src, 3, 5), src)
    for Cin, (kw, pw, kwp) in itertools.product(T.PAIR_CIN, T.PAIR_GEOMS):
        wq = _ints((5, Cin, 3, kw), 22) + 10.0           # no zero among the values
        wp = V.weight_pairs(wq, pw, kwp)
        assert torch.equal(V.weight_pairs_bwd(wp, Cin, kw, pw), wq)
        assert int((wp != 0).sum()) == wq.numel() and wp.sum() == wq.sum()      # every weight exactly once
    x = _ints((2, 3, 3, 6), 23)
    assert torch.equal(V.nhwc_pad8(x).reshape(2, 3, 6, 8)[..., :3].permute(0, 3, 1, 2), x) and V.nhwc_pad8(x).sum() == x.sum()
    assert torch.equal(V.nhwc_pair4(x).reshape(2, 3, 3, 2, 4)[..., :3].reshape(2, 3, 6, 3).permute(0, 3, 1, 2), x)


def test_pair_weights_are_the_stride_2_convolution_over_pixel_pairs():
    """the [N, H, W/2, 8] pair view convolved with the pair weights at stride (sh, 1), padding (ph, (pw + (pw & 1)) / 2), is
    the stride-(sh, 2) convolution of the map"""
    N, Cin, Cout, H, W = 2, 3, 5, 6, 12
    for kw, pw, kwp in T.PAIR_GEOMS:
        w, x = _ints((Cout, Cin, 3, kw), 24), _ints((N, Cin, H, W), 25)
        want = TF.conv2d(x, w, stride=(2, 2), padding=(1, pw))
        pairs = V.nhwc_pair4(x).reshape(N, H, W // 2, 8).permute(0, 3, 1, 2)
        got = TF.conv2d(pairs, V.weight_pairs(w, pw, kwp), stride=(2, 1), padding=(1, (pw + (pw & 1)) // 2))
        assert torch.equal(got[..., :want.shape[3]], want), (kw, pw, kwp)


def test_grouped_pack_forms():
    w = _ints((5, 3, 3, 2), 30) + 10.0
    assert torch.equal(V.weight_pack_group(w, 0, 5, 3, 24), V.weight_pack(w, 24))
    assert torch.equal(V.weight_pack_group(w, 1, 5, 3), V.weight_pack_dgrad(w))
    assert torch.equal(V.weight_pack_group(w, 2, 5, 3, cls=(1, 1, 0, 0)), V.weight_pack_dgrad(w))   # stride 1: one class, all taps
    big0, big1 = V.weight_pack_group(w, 0, 8, 4, 30), V.weight_pack_group(w, 1, 8, 4)
    assert big0.shape == (8, 30) and big1.shape == (4, 6 * 8) and big0.sum() == w.sum() == big1.sum()
    assert torch.equal(big0[:, :24].reshape(8, 6, 4)[:5, :, :3], V.weight_pack(w, 18).reshape(5, 6, 3)) and not big0[:, 24:].any()
    assert torch.equal(big1.reshape(4, 6, 8)[:3, :, :5], V.weight_pack_dgrad(w).reshape(3, 6, 5))
    # the classes of one layer hold every tap exactly once, each class in decreasing tap order
    for (kh, kw), (sh, sw) in (((3, 3), (2, 2)), ((3, 2), (2, 1)), ((7, 7), (2, 2)), ((1, 1), (2, 2))):
        wq = torch.arange(1, 4 * 3 * kh * kw + 1, dtype=F64).reshape(4, 3, kh, kw)
        seen = []
        for rh, rw in itertools.product(range(min(sh, kh)), range(min(sw, kw))):
            out = V.weight_pack_group(wq, 2, 6, 5, cls=(sh, sw, rh, rw))
            nth, ntw = len(V.class_taps(kh, rh, sh)), len(V.class_taps(kw, rw, sw))
            assert out.shape == (5, nth * ntw * 6)
            blk = out.reshape(5, nth, ntw, 6)
            assert not blk[3:].any() and not blk[..., 4:].any()
            for j, l in itertools.product(range(nth), range(ntw)):
                ki, kj = rh + (nth - 1 - j) * sh, rw + (ntw - 1 - l) * sw
                assert torch.equal(blk[:3, j, l, :4], wq[:, :, ki, kj].t())
            seen += blk[blk != 0].tolist()
        assert sorted(seen) == wq.flatten().tolist()


def test_strided_data_gradient_from_the_parity_classes():
    """the gradient at the input pixels of one parity class is a stride-1 convolution of dz with that class's taps"""
    Cout, Cin, kh, kw, sh, sw, ph, pw, H, W = 4, 3, 3, 3, 2, 2, 1, 1, 8, 10
    w = _ints((Cout, Cin, kh, kw), 31)
    x = _ints((1, Cin, H, W), 32).requires_grad_(True)
    y = TF.conv2d(x, w, stride=(sh, sw), padding=(ph, pw))
    dz = _ints(tuple(y.shape), 33)
    dx, = torch.autograd.grad(y, x, dz)
    for a, b in itertools.product(range(sh), range(sw)):
        rh, rw = (a + ph) % sh, (b + pw) % sw
        nth, ntw = len(V.class_taps(kh, rh, sh)), len(V.class_taps(kw, rw, sw))
        wd = V.weight_pack_group(w, 2, Cout, Cin, cls=(sh, sw, rh, rw)).reshape(Cin, nth, ntw, Cout).permute(0, 3, 1, 2)
        full = TF.conv2d(dz, wd, padding=(nth - 1, ntw - 1))          # every alignment of the class taps over dz
        want = dx[0, :, a::sh, b::sw]
        # pixel hi = a + sh*q reads dz rows (hi + ph - ki) / sh for the class taps: the largest tap first, row q + (a+ph-rh)/sh - (nth-1)
        oh, ow = (a + ph - rh) // sh, (b + pw - rw) // sw
        got = full[0, :, oh:oh + want.shape[1], ow:ow + want.shape[2]]
        assert torch.equal(got, want), (a, b)


# ---------------------------------------------------------------- sensitivity
def _share(a, b):
    """share of elements that differ (a NaN differs from everything)"""
    return float((a.reshape(-1) != b.reshape(-1)).double().mean())


def test_the_operands_expose_every_index_slip():
    """each fault applied to the statement changes at least MIN of the expected output at the operands of the GPU cases (all
    geometries asymmetric: kh != kw, sh != sw, ph != pw, H != W, Cin != Cout, values that differ per channel and position).
    MIN = 1/4: each of these slips moves whole tap blocks, rows or columns of the output, i.e. a constant fraction of it well
    above a quarter, and the operands take thousands of distinct values, so coincidences are a few elements at most."""
    MIN = 0.25
    N = T.N
    shares = {}
    C, H, W, k, s, p, extra = T.IM2COL_GEOMS[0]
    assert len({*V.pair(k)}) == len({*V.pair(s)}) == len({*V.pair(p)}) == 2 and H != W
    K = T._K(C, k)
    for nchw in (False, True):
        x = V.move_values((N, C, H, W) if nchw else (N, H, W, C), torch.float32, 100)
        good = V.im2col(x, nchw, N, C, H, W, k, s, p, K + extra)
        for f in ("ki_kj_swapped", "pad_h", "pad_w", "stride_swapped"):
            shares[f"im2col nchw={nchw} {f}"] = _share(good[:, :K], V.im2col(x, nchw, N, C, H, W, k, s, p, K + extra, fault=f)[:, :K])
    C, H, W, k, s, p, extra, _ = T.C2I_SCALAR["c5"]
    Ho, Wo = V.out_hw(H, W, k, s, p)
    K = T._K(C, k)
    d = T._dcol(N * Ho * Wo, K, K + extra, V.c2i_bound(k, s, False, torch.bfloat16), 210)
    good = V.col2im(d, N, C, H, W, k, s, p)
    for f in ("ki_kj_swapped", "pad_h", "pad_w", "stride_swapped", "k_padding_read"):
        shares[f"col2im {f}"] = _share(good, V.col2im(d, N, C, H, W, k, s, p, fault=f))
    C, H, W, k, s, p, extra, add = T.C2I_VEC["c16-add-compact"]
    assert add == "compact" and H % 2 and W % 2
    Ho, Wo = V.out_hw(H, W, k, s, p)
    bound = V.c2i_bound(k, s, True, torch.bfloat16)
    d = T._dcol(N * Ho * Wo, T._K(C, k), T._K(C, k) + extra, bound, 200)
    a, st = T._add_operand(add, C, H, W, bound, 201)
    shares["col2im add_on_odd_pixels"] = _share(V.col2im(d, N, C, H, W, k, s, p, add=a, add_stride=st),
                                                V.col2im(d, N, C, H, W, k, s, p, add=a, add_stride=st, fault="add_on_odd_pixels"))
    Cout, Cin, kh, kw = T.W_SHAPE
    assert Cout != Cin and kh != kw
    w = V.move_values(T.W_SHAPE, torch.float32, 301)
    for f in ("not_rotated", "rotated_h_only", "rotated_w_only", "channels_not_transposed"):
        shares[f"dgrad {f}"] = _share(V.weight_pack_dgrad(w), V.weight_pack_dgrad(w, fault=f))
    g = torch.full((Cout, Cin * kh * kw + 6), float("nan"), dtype=F64)
    g[:, :Cin * kh * kw] = V.int_values((Cout, Cin * kh * kw), 1000, 310)
    shares["unpack k_padding_read"] = _share(V.weight_unpack(g, T.W_SHAPE), V.weight_unpack(g, T.W_SHAPE, fault="k_padding_read"))
    for Cin, (kw, pw, kwp) in itertools.product(T.PAIR_CIN, T.PAIR_GEOMS):
        w = V.move_values((5, Cin, 3, kw), torch.float32, 330 + Cin)
        nonzero = Cin / 4.0 * kw / (2 * kwp)                        # the share of wp that holds a weight at all
        shares[f"pairs off_flipped Cin={Cin} kw={kw} pw={pw}"] = min(1.0, _share(V.weight_pairs(w, pw, kwp), V.weight_pairs(w, pw, kwp, fault="off_flipped")) / nonzero)
        vals = V.int_values((5, 8, 3, kwp), 1000, 340 + Cin)
        shares[f"pairs_bwd off_flipped Cin={Cin} kw={kw} pw={pw}"] = _share(V.weight_pairs_bwd(vals, Cin, kw, pw),
                                                                           V.weight_pairs_bwd(vals, Cin, kw, pw, fault="off_flipped"))
    for what, share in shares.items():
        print(f"{what}: {share:.3f} of the expected output changes")
    low = {k: v for k, v in shares.items() if v < MIN}
    assert not low, low


def test_the_move_operands_hold_the_special_values():
    for name, dtype in V.DTYPES.items():
        x = V.move_values((2, 5, 7, 10), dtype, 1)
        assert torch.equal(x.to(dtype).double(), x), name
        flat = x.flatten()
        assert (flat == 0).sum() >= 4 and torch.signbit(flat[flat == 0]).any() and not torch.signbit(flat[flat == 0]).all()
        assert flat.max() == torch.finfo(dtype).max and flat.min() == -torch.finfo(dtype).max
        assert len(flat.unique()) > flat.numel() * (0.9 if dtype == torch.float32 else 0.3)
    x = V.move_values((2, 5, 7, 10), torch.float32, 1).flatten()
    for dst, tie in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        ulp = 2 * tie
        assert (x == 1 + tie).any() and (x == 1 + 3 * tie).any()                       # halfway, even below and even above
        assert float(torch.tensor(1 + tie).to(dst)) == 1.0 and float(torch.tensor(1 + 3 * tie).to(dst)) == 1 + 2 * ulp
        assert (x.to(dst).double() != x).double().mean() > 0.9                           # the conversion really rounds
    assert torch.isinf(torch.tensor(torch.finfo(torch.float32).max).to(torch.bfloat16))    # the top of fp32 rounds to infinity
    a = torch.tensor([0.0, -0.0, 1.0])
    assert V.same_bits(a, a.clone()) and not V.same_bits(a, torch.tensor([0.0, 0.0, 1.0]))


# ---------------------------------------------------------------- the tables reach what they name
def test_the_mirrors_restate_the_sources_constants():
    assert V.conv_hip_constants() == {"PACK_GROUP": V.PACK_GROUP, "PACK_ROW_MAX": V.PACK_ROW_MAX, "BLOCK": V.BLOCK,
                                      "GRID_BLOCKS_PER_CU": V.GRID_BLOCKS_PER_CU}


def test_the_shape_tables_reach_what_they_are_there_for():
    K = T._K
    # im2col: the general kernel for every pair and layout; the fallbacks are one condition away from the other two
    for (src, dst), nchw in itertools.product(V.PAIRS7, (False, True)):
        for C, H, W, k, s, p, extra in T.IM2COL_GEOMS:
            assert V.im2col_route(src, dst, nchw, C, k, K(C, k) + extra, True) == f"im2col_kernel<{V.CXX[src]}, {V.CXX[dst]}, {'true' if nchw else 'false'}>"
    C, H, W, k, s, p, _ = T.IM2COL_GEOMS[1]
    assert (H + 2 * p - k) % s and (W + 2 * p - k) % s
    C, H, W, k, s, p, _ = T.IM2COL_GEOMS[2]
    assert (k, s, p) == (1, 2, 0) and H % 2 and W % 2
    near = {"nchw3k7-ld147": dict(ld=152), "nhwc8-ldpad8": dict(extra=0), "nhwc8-misaligned": dict(aligned=True), "nhwc8-converting": dict(dst="fp32")}
    for name, (src, dst, nchw, C, H, W, k, s, p, extra, mis) in T.IM2COL_FALLBACKS.items():
        ld = K(C, k) + extra
        assert V.im2col_route(src, dst, nchw, C, k, ld, not mis).startswith("im2col_kernel<"), name
        fix = near[name]
        other = V.im2col_route(src, fix.get("dst", dst), nchw, C, k, fix.get("ld", K(C, k) + fix.get("extra", extra)), fix.get("aligned", not mis))
        assert other.startswith("im2col_nchw_stem_kernel<" if nchw else "im2col_nhwc_vec_kernel<"), name
    assert T.IM2COL_FALLBACKS["nchw3k7-ld147"][9] == 0 and 147 % 8
    for src, dst in V.PAIRS7:
        for H, W, s, p, ld in T.STEM_GEOMS:
            assert V.im2col_route(src, dst, True, 3, 7, ld, True) == f"im2col_nchw_stem_kernel<{V.CXX[src]}, {V.CXX[dst]}, 3, 7, 7>"
    lds = [g[4] for g in T.STEM_GEOMS]
    assert any(0 < ld - 147 < 8 for ld in lds) and any(ld - 147 >= 8 + (-147) % 8 for ld in lds)
    assert any(V.pair(g[2])[0] != V.pair(g[2])[1] and V.pair(g[3])[0] != V.pair(g[3])[1] for g in T.STEM_GEOMS)
    for n, C in itertools.product(V.NAMES, T.VEC_WIDTHS):
        assert V.im2col_route(n, n, False, C, T.VEC_GEOM[2], K(C, T.VEC_GEOM[2]), True) == f"im2col_nhwc_vec_kernel<{V.CXX[n]}>"
    # col2im
    for n in V.NAMES:
        for name, (C, H, W, k, s, p, extra, add) in T.C2I_VEC.items():
            assert V.col2im_route(n, C, K(C, k) + extra, True, add is not None) == f"col2im_nhwc_kernel<{V.CXX[n]}>", name
            assert V.c2i_bound(k, s, add is not None, V.DTYPES[n]) >= 8
        for name, (C, H, W, k, s, p, extra, mis) in T.C2I_SCALAR.items():
            assert V.col2im_route(n, C, K(C, k) + extra, not mis) == f"col2im_scalar_kernel<{V.CXX[n]}, {V.CXX[n]}, false>", name
            assert V.c2i_bound(k, s, False, V.DTYPES[n]) >= 8
        assert V.col2im_route(n, 5, 45, True, add=True) == "unsupported"
    vec = T.C2I_VEC
    assert {v[0] for v in vec.values()} == {8, 16} and any(v[6] == 8 for v in vec.values())
    assert {v[7] for v in vec.values()} == {None, "full", "compact"} and any(v[3:6] == (1, 2, 0) for v in vec.values())
    C, H, W, k, s, p, extra, add = vec["c16-add-compact"]
    assert add == "compact" and H % 2 and W % 2
    sc = T.C2I_SCALAR
    assert sc["c8-misaligned"][0] % 8 == 0 and sc["c8-misaligned"][7] and sc["c5"][0] % 8
    for name, taps_per_row in (("kw7-sw1", 7), ("kw7-sw2", 4)):
        (kh, kw), (sh, sw) = V.pair(sc[name][3]), V.pair(sc[name][4])
        assert -(-kw // sw) == taps_per_row                     # > 4: a second trip of the four-tap batch; == 4: exactly one
    C, H, W, k, s, p, extra, _ = sc["edges"]
    (kh, kw), (sh, sw), (ph, pw) = V.pair(k), V.pair(s), V.pair(p)
    Ho, _ = V.out_hw(H, W, k, s, p)
    walked = [(h, ki) for h in range(H) for ki in range((h + ph) % sh, kh, sh)]
    assert any(h + ph - ki >= 0 and (h + ph - ki) // sh >= Ho for h, ki in walked) and any(h + ph - ki < 0 for h, ki in walked)
    assert V.col2im_nchw_route("bf16", "fp32") == "col2im_scalar_kernel<std::bfloat16_t, float, true>"
    assert T.C2I_NCHW[6] > K(T.C2I_NCHW[0], T.C2I_NCHW[3])
    # the grouped pack: every form, both load branches of rows and tile, both store branches of each 16-bit form
    reached = set()
    for name, rows in T.PACK_GROUP_CASES.items():
        for (co, ci, kh, kw, cop, cip, ld, kind, cls, mis), n in itertools.product(rows, V.NAMES):
            form, R, blocks, load, store = V.pack_plan(co, ci, kh, kw, cop, cip, ld, kind, n, src_aligned=not mis)
            reached.add((form, load, store, n != "fp32"))
            assert blocks >= 1
            if name.startswith("kind2"):
                assert kind == 2 and form == "tile"
            if name == "elems-rowlen":
                assert form == "elems" and ci * kh * kw > V.PACK_ROW_MAX and ld <= 4 * V.PACK_ROW_MAX
            if name == "elems-ld":
                assert form == "elems" and ci * kh * kw <= V.PACK_ROW_MAX and ld > 4 * V.PACK_ROW_MAX
            if name == "misaligned-src":
                assert load == "scalar" and (ci * kh * kw) % 4 == 0 and V.pack_plan(co, ci, kh, kw, cop, cip, ld, kind, n)[3] == "vec"
            if name == "scalar-store-cin":
                assert form == "rows" and store == "scalar" and cip % 8 and ld % 8 == 0
            if name == "scalar-store-cout":
                assert form == "tile" and store == "scalar" and cop % 8
            if name == "rows-r1":
                assert form == "rows" and R == 1 and ld >= 2048
            if name == "rows-r3-ragged":
                assert form == "rows" and R > 1 and cop % R and ld < 2048 and co < cop
    for form in ("rows", "tile"):
        assert {(form, l, s, True) for l in ("vec", "scalar") for s in ("vec", "scalar")} >= {r for r in reached if r[0] == form and r[3]}
        assert {r[1] for r in reached if r[0] == form} == {"vec", "scalar"}
        assert {r[2] for r in reached if r[0] == form and r[3]} == {"vec", "scalar"}
    assert {tuple(r[8][:2]) for rows in T.PACK_GROUP_CASES.values() for r in rows if r[7] == 2} == {(2, 2), (2, 1)}
    assert {tuple(r[8][2:]) for r in T.PACK_GROUP_CASES["kind2-s22"]} == set(itertools.product((0, 1), repeat=2))
    # layouts and pair weights
    for (src, dst), cpad in itertools.product(V.PAIRS6, (4, 8)):
        assert V.nhwc_pad_route(src, dst, cpad).startswith("nchw_to_nhwc_p")
    assert max(T.NHWC_PAD8[0]) == 8 and max(T.NHWC_PAIR4[0]) == 4 and T.NHWC_PAIR4[2] % 2 == 0 and T.NHWC_PAD8[2] % 2
    assert {pw & 1 for _, pw, _ in T.PAIR_GEOMS} == {0, 1} and all(2 * kwp - (pw & 1) >= kw for kw, pw, kwp in T.PAIR_GEOMS)
    assert any(2 * kwp - (pw & 1) > kw for kw, pw, kwp in T.PAIR_GEOMS)           # a pair position outside the kernel
    # the grid cap: just past one trip of the capped grid, whatever the device's CU count
    for cus, family in itertools.product((64, 256, 304), T.GRID_CAP):
        cap = V.grid_cap(cus)
        items, q = T.grid_cap_call(family, cap)
        assert cap < items < cap + V.BLOCK and (items - cap) % V.BLOCK, (family, cus)
    W = T.grid_cap_call("im2col_vec", V.grid_cap(256))[1]["W"]
    assert V.im2col_route("bf16", "bf16", False, 8, (1, 2), 16, True) == "im2col_nhwc_vec_kernel<std::bfloat16_t>" and W > 0
    assert V.im2col_route("bf16", "bf16", True, 3, 7, 152, True).startswith("im2col_nchw_stem")
    assert V.col2im_route("bf16", 8, 16, True).startswith("col2im_nhwc") and V.col2im_route("bf16", 1, 2, True).startswith("col2im_scalar")


# ---------------------------------------------------------------- argument validation (no launch: N = 0)
def test_col2im_entry_points_refuse_what_im2col_refuses():
    from dvt_amd import _lib
    lib = _lib.load()
    P, Q = 4096, 8192                                    # non-null; N = 0, so nothing is ever read or written
    ok = dict(C=8, H=7, W=10, kh=3, kw=3, ld=72)
    bad = [dict(H=0), dict(H=-1), dict(W=0), dict(kh=0), dict(kw=0), dict(kw=-3), dict(ld=71), dict(ld=0), dict(C=0),
           dict(H=1, kh=5), dict(W=1, kw=5)]                                     # the last two: no output position at all

    def im2col(a):
        return lib.dvt_im2col(P, _lib.BF16, 0, Q, _lib.BF16, 0, a["C"], a["H"], a["W"], a["kh"], a["kw"], 2, 2, 1, 1, a["ld"], None)

    def col2im(a):
        return lib.dvt_col2im(P, Q, 0, a["C"], a["H"], a["W"], a["kh"], a["kw"], 2, 2, 1, 1, a["ld"], None, 0, _lib.BF16, None)

    def col2im_nchw(a):
        return lib.dvt_col2im_nchw(P, _lib.BF16, Q, _lib.F32, 0, a["C"], a["H"], a["W"], a["kh"], a["kw"], 2, 2, 1, 1, a["ld"], None)

    for fn in (im2col, col2im, col2im_nchw):
        assert fn(ok) == 0, fn.__name__
        for change in bad:
            assert fn({**ok, **change}) == -1, (fn.__name__, change)
    assert b"ld smaller" in lib.dvt_last_error() or b"col2im" in lib.dvt_last_error()
    assert lib.dvt_col2im(None, Q, 0, 8, 7, 10, 3, 3, 2, 2, 1, 1, 72, None, 0, _lib.BF16, None) == -1
    assert lib.dvt_col2im(P, Q, 0, 8, 7, 10, 3, 3, 0, 2, 1, 1, 72, None, 0, _lib.BF16, None) == -1
    assert lib.dvt_col2im(P, Q, 0, 8, 7, 10, 3, 3, 2, 2, 1, -1, 72, None, 0, _lib.BF16, None) == -1
    assert lib.dvt_col2im(P, Q, 0, 8, 7, 10, 3, 3, 2, 2, 1, 1, 72, None, -2, _lib.BF16, None) == -1
    assert lib.dvt_col2im_nchw(P, _lib.BF16, None, _lib.F32, 0, 3, 9, 12, 7, 7, 2, 2, 3, 3, 152, None) == -1
    # the second gradient path without the vector route: the unsupported code
    assert lib.dvt_col2im(P, Q, 0, 5, 7, 10, 3, 3, 2, 2, 1, 1, 45, Q, 0, _lib.BF16, None) == -2
    assert lib.dvt_col2im(P, Q, 0, 8, 7, 10, 3, 3, 2, 2, 1, 1, 72, Q + 2, 0, _lib.BF16, None) == -2
