"""Plain statements of the data-movement kernels of csrc/conv.hip -- im2col, col2im, the weight forms, pad / unpad, the
pixel-pair weights and the two NCHW -> NHWC layouts -- by index arithmetic in whatever floating dtype they are handed
(float64: the reference; float32: the chain the col2im sums are judged against under tests/rowwise_ref.py), the operands of
tests/test_gpu_conv_data.py, and the dispatch mirrors tests/test_conv_data_coverage.py derives template arguments from.
No GPU is touched here; tests/test_conv_data_cpu.py anchors this file on torch's unfold / fold / conv2d.

Every statement is written from the comment above its kernel, not from the kernel's loop: im2col as "for each tap, the
shifted window of the map", col2im as the scatter-add adjoint of that (the kernels gather), the weight forms as slices of
the parameter per tap.  ``fault=`` applies one named slip to a statement (tests/test_conv_data_cpu.py proves that the
operands of the GPU cases expose each of them); no kernel is involved in that.

Exactness.  The move kernels convert once: the expected output is the float64 operand rounded to the output dtype (round to
nearest even), compared bit for bit (so that -0.0 is not taken for +0.0).  The col2im sums get integer operands bounded by
``c2i_bound`` so that the largest possible sum -- ceil(kh/sh) * ceil(kw/sw) taps, one more with the add path -- is exact in
the output dtype (``gemm_exact.check_bound``): equality then holds in any summation order."""
from __future__ import annotations

import math
import os
import re

import torch

from tests.gemm_exact import LIMIT, check_bound, small_ints          # noqa: F401  (re-exported for the test files)

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CXX = {"fp32": "float", "bf16": "std::bfloat16_t", "fp16": "_Float16"}
NAMES = list(DTYPES)
# (source, destination) pairs the converting kernels are instantiated for
PAIRS7 = [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "fp32"),
          ("fp16", "fp32")]
PAIRS6 = [("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "fp16"), ("fp16", "bf16")]
_IVIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}

PACK_GROUP = 40            # entries per launch of weight_pack_group_kernel
PACK_ROW_MAX = 8192        # words of a parameter row the LDS forms hold
BLOCK = 256
GRID_BLOCKS_PER_CU = 8


def pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_hw(H, W, k, stride, pad):
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def pair_id(p):
    return f"{p[0]}-{p[1]}"


# ---------------------------------------------------------------- im2col / col2im
def _nhwc(x, nchw, N, C, H, W):
    return x.reshape(N, C, H, W).permute(0, 2, 3, 1) if nchw else x.reshape(N, H, W, C)


def _window(n_out, size, s, p, kk):
    """input coordinate of every output position for tap kk, and which of them lie inside the map"""
    pos = torch.arange(n_out) * s - p + kk
    return pos, (pos >= 0) & (pos < size)


def im2col(x, nchw, N, C, H, W, k, stride, pad, ld, fault=None):
    """out[(n, ho, wo), (ki*kw + kj)*C + c] = x[n, ho*sh - ph + ki, wo*sw - pw + kj, c], zero outside the map and in the
    columns [kh*kw*C, ld)"""
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    Ho, Wo = out_hw(H, W, k, stride, pad)
    xs = _nhwc(x, nchw, N, C, H, W)
    if fault == "stride_swapped":
        sh, sw = sw, sh
    ph, pw = ph + (fault == "pad_h"), pw + (fault == "pad_w")
    out = torch.zeros(N, Ho, Wo, ld, dtype=x.dtype)
    for ki in range(kh):
        for kj in range(kw):
            hs, okh = _window(Ho, H, sh, ph, ki)
            ws, okw = _window(Wo, W, sw, pw, kj)
            win = xs[:, hs.clamp(0, H - 1)][:, :, ws.clamp(0, W - 1)]
            inside = (okh[:, None] & okw[None, :])[None, :, :, None]
            col = ((kj * kh + ki) if fault == "ki_kj_swapped" else (ki * kw + kj)) * C
            out[..., col:col + C] = torch.where(inside, win, torch.zeros((), dtype=x.dtype))
    return out.reshape(N * Ho * Wo, ld)


def col2im(dcol, N, C, H, W, k, stride, pad, add=None, add_stride=0, nchw=False, fault=None):
    """the adjoint, as a scatter-add: every column block of every row of dcol [N*Ho*Wo, ld] is added to the pixel its tap
    read; the columns [kh*kw*C, ld) are never read.  add: a second path, [N*H*W, C] (add_stride 0) or the compact
    [N*ceil(H/s)*ceil(W/s), C] added at the pixels h % s == 0 and w % s == 0.  -> [N*H*W, C], or [N, C, H, W] (nchw)"""
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(stride), pair(pad)
    Ho, Wo = out_hw(H, W, k, stride, pad)
    ld = dcol.shape[1]
    if fault == "k_padding_read":                        # the rows taken as kh*kw*C long: the padding columns slide in
        d = dcol.reshape(-1)[:N * Ho * Wo * kh * kw * C].reshape(N, Ho, Wo, kh * kw * C)
    else:
        d = dcol.reshape(N, Ho, Wo, ld)
    if fault == "stride_swapped":
        sh, sw = sw, sh
    ph, pw = ph + (fault == "pad_h"), pw + (fault == "pad_w")
    dx = torch.zeros(N, H, W, C, dtype=dcol.dtype)
    for ki in range(kh):
        for kj in range(kw):
            hs, okh = _window(Ho, H, sh, ph, ki)
            ws, okw = _window(Wo, W, sw, pw, kj)
            ho, wo = okh.nonzero().flatten(), okw.nonzero().flatten()
            if not len(ho) or not len(wo):
                continue
            col = ((kj * kh + ki) if fault == "ki_kj_swapped" else (ki * kw + kj)) * C
            # distinct output positions land on distinct pixels (stride >= 1): a plain indexed += adds each once
            dx[:, hs[ho][:, None], ws[wo][None, :]] += d[:, ho[:, None], wo[None, :], col:col + C]
    if add is not None:
        if add_stride == 0:
            dx += add.reshape(N, H, W, C)
        else:
            s = add_stride
            Hs, Ws = -(-H // s), -(-W // s)
            a = add.reshape(N, Hs, Ws, C)
            if fault == "add_on_odd_pixels":
                dx[:, 1::s, 1::s] += a[:, :len(range(1, H, s)), :len(range(1, W, s))]
            else:
                dx[:, ::s, ::s] += a
    return dx.permute(0, 3, 1, 2).contiguous() if nchw else dx.reshape(N * H * W, C)


def c2i_taps(k, stride, add=False):
    """the most terms a pixel's sum can have"""
    (kh, kw), (sh, sw) = pair(k), pair(stride)
    return -(-kh // sh) * -(-kw // sw) + int(add)


def c2i_bound(k, stride, add, *dtypes):
    """largest operand magnitude with which every sum stays exact in every one of ``dtypes``"""
    return min(LIMIT[d] for d in dtypes) // c2i_taps(k, stride, add)


# ---------------------------------------------------------------- weight forms
def weight_pack(w, ld):
    """dst[co, (ki*kw + kj)*Cin + ci] = w[co, ci, ki, kj]; columns from kh*kw*Cin on are zero"""
    Cout, Cin, kh, kw = w.shape
    dst = torch.zeros(Cout, ld, dtype=w.dtype)
    for ki in range(kh):
        for kj in range(kw):
            col = (ki * kw + kj) * Cin
            dst[:, col:col + Cin] = w[:, :, ki, kj]
    return dst


def weight_unpack(g, shape, fault=None):
    """dw[co, ci, ki, kj] = g[co, (ki*kw + kj)*Cin + ci] of g [Cout, ld]; the columns from kh*kw*Cin on are never read"""
    Cout, Cin, kh, kw = shape
    K = kh * kw * Cin
    rows = g.reshape(-1)[:Cout * K].reshape(Cout, K) if fault == "k_padding_read" else g
    dw = torch.zeros(Cout, Cin, kh, kw, dtype=g.dtype)
    for ki in range(kh):
        for kj in range(kw):
            col = (ki * kw + kj) * Cin
            dw[:, :, ki, kj] = rows[:, col:col + Cin]
    return dw


def weight_unpack_t(gt, shape):
    """dw[co, ci, ki, kj] = gt[(ki*kw + kj)*Cin + ci, co] of gt [kh*kw*Cin, Cout]"""
    Cout, Cin, kh, kw = shape
    dw = torch.zeros(Cout, Cin, kh, kw, dtype=gt.dtype)
    for ki in range(kh):
        for kj in range(kw):
            row = (ki * kw + kj) * Cin
            dw[:, :, ki, kj] = gt[row:row + Cin].t()
    return dw


def weight_pack_dgrad(w, fault=None):
    """dst[ci, ((kh-1-ki)*kw + (kw-1-kj))*Cout + co] = w[co, ci, ki, kj]: taps rotated by 180 degrees, channels transposed"""
    Cout, Cin, kh, kw = w.shape
    if fault == "channels_not_transposed":               # [Cout, taps * Cin] written into the same number of elements
        dst = torch.zeros(Cout, kh * kw * Cin, dtype=w.dtype)
        for ki in range(kh):
            for kj in range(kw):
                col = ((kh - 1 - ki) * kw + (kw - 1 - kj)) * Cin
                dst[:, col:col + Cin] = w[:, :, ki, kj]
        return dst.reshape(Cin, kh * kw * Cout)
    dst = torch.zeros(Cin, kh * kw * Cout, dtype=w.dtype)
    for ki in range(kh):
        for kj in range(kw):
            ri = ki if fault in ("not_rotated", "rotated_w_only") else kh - 1 - ki
            rj = kj if fault in ("not_rotated", "rotated_h_only") else kw - 1 - kj
            col = (ri * kw + rj) * Cout
            dst[:, col:col + Cout] = w[:, :, ki, kj].t()
    return dst


def class_taps(k, r, s):
    """taps r, r + s, ... below k of one parity class"""
    return list(range(r, k, s))


def weight_pack_group(w, kind, cout_p, cin_p, ld=0, cls=None):
    """one entry of the grouped pack, w [cout_l, cin_l, kh, kw], zero-extended to cout_p / cin_p channels:
    kind 0 -> [cout_p, ld], column tap*cin_p + ci, zeros from kh*kw*cin_p on;
    kind 1 -> [cin_p, kh*kw*cout_p], destination tap kh*kw - 1 - tap (the rotation), channels transposed;
    kind 2 -> [cin_p, nth*ntw*cout_p]: only the taps ki = rh + j*sh, kj = rw + l*sw of cls = (sh, sw, rh, rw), the largest
              ki / kj first"""
    cout_l, cin_l, kh, kw = w.shape
    if kind == 0:
        dst = torch.zeros(cout_p, ld, dtype=w.dtype)
        for ki in range(kh):
            for kj in range(kw):
                col = (ki * kw + kj) * cin_p
                dst[:cout_l, col:col + cin_l] = w[:, :, ki, kj]
        return dst
    if kind == 1:
        his, wis = list(range(kh)), list(range(kw))
    else:
        sh, sw, rh, rw = cls
        his, wis = class_taps(kh, rh, sh), class_taps(kw, rw, sw)
    dst = torch.zeros(cin_p, len(his), len(wis), cout_p, dtype=w.dtype)
    for j, ki in enumerate(reversed(his)):
        for l, kj in enumerate(reversed(wis)):
            dst[:cin_l, j, l, :cout_l] = w[:, :, ki, kj].t()
    return dst.reshape(cin_p, len(his) * len(wis) * cout_p)


def pad3(src, Ap, Bp):
    A, B, K = src.shape
    dst = torch.zeros(Ap, Bp, K, dtype=src.dtype)
    dst[:A, :B] = src
    return dst


def unpad3(src, A, B):
    return src[:A, :B].clone()


def weight_pairs(w, pw, kwp, fault=None):
    """wp[co, px*4 + c, ki, p] = w[co, c, ki, 2p - off + px], off = pw & 1; zero outside 0 <= kj < kw and for c >= Cin"""
    Cout, Cin, kh, kw = w.shape
    off = (pw & 1) ^ (fault == "off_flipped")
    wp = torch.zeros(Cout, 8, kh, kwp, dtype=w.dtype)
    for p in range(kwp):
        for px in range(2):
            kj = 2 * p - off + px
            if 0 <= kj < kw:
                wp[:, px * 4:px * 4 + Cin, :, p] = w[:, :, :, kj]
    return wp


def weight_pairs_bwd(dwp, Cin, kw, pw, fault=None):
    """the adjoint gather: dw[co, c, ki, kj] = dwp[co, px*4 + c, ki, p] with 2p + px = kj + off"""
    Cout, _, kh, kwp = dwp.shape
    off = (pw & 1) ^ (fault == "off_flipped")
    dw = torch.zeros(Cout, Cin, kh, kw, dtype=dwp.dtype)
    for kj in range(kw):
        p, px = (kj + off) >> 1, (kj + off) & 1
        if p < kwp:                                      # always, unless the fault shifted the last column out
            dw[:, :, :, kj] = dwp[:, px * 4:px * 4 + Cin, :, p]
    return dw


# ---------------------------------------------------------------- layouts
def nhwc_pad8(x):
    """[N, C, H, W] -> [N*H*W, 8]: channel c of a pixel in column c, zeros from C on"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, 8, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y.reshape(N * H * W, 8)


def nhwc_pair4(x):
    """[N, C, H, W], W even -> [N*H*(W/2), 8]: pixel 2j of a row in columns 0..3, pixel 2j + 1 in columns 4..7"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W // 2, 2, 4, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 1).reshape(N, H, W // 2, 2, C)
    return y.reshape(N * H * (W // 2), 8)


# ---------------------------------------------------------------- operands
def rounded_to(ref64, dtype):
    """the float64 statement rounded once to the output dtype (round to nearest even)"""
    return ref64.to(dtype)


def same_bits(got, want):
    """torch.equal, and the same bit patterns (so -0.0 is told from +0.0); the expected tensor has no NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.equal(got, want) and torch.equal(got.contiguous().view(_IVIEW[got.dtype]), want.contiguous().view(_IVIEW[want.dtype]))


def specials(src_dtype):
    """values a converting move must get right: signed zeros, the rounding ties of bf16 and fp16 (either neighbour even), and
    the largest finite value of the source type -- rounded to the source type, as every operand is"""
    top = torch.finfo(src_dtype).max
    v = [0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11),
         top, -top]
    return torch.tensor(v, dtype=torch.float64).to(src_dtype).double()


def move_values(shape, src_dtype, seed):
    """float64 values on the grid of ``src_dtype``: a different value at (nearly) every position and per channel -- 24-bit
    random mantissas, so that a conversion to 16 bits really rounds -- with ``specials`` written over the first elements and
    again over the last ones"""
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    x = ((torch.rand(n, generator=g, dtype=torch.float64) * 7.0 + 0.5) *
         torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()).to(src_dtype).double()
    sp = specials(src_dtype)
    m = min(len(sp), n // 2)
    x[:m] = sp[:m]
    x[n - m:] = sp[:m].flip(0)
    return x.reshape(shape)


def int_values(shape, bound, seed):
    """integers in [-bound, bound], float64"""
    return small_ints(shape, -bound, bound, seed)


# ---------------------------------------------------------------- dispatch mirrors
def im2col_route(x_dtype, out_dtype, nchw, C, k, ld, aligned):
    """the symbol dvt_im2col launches.  aligned: both buffers start on a 16-byte boundary"""
    kh, kw = pair(k)
    S, D = CXX[x_dtype], CXX[out_dtype]
    assert (x_dtype, out_dtype) in PAIRS7
    if nchw and C == 3 and (kh, kw) == (7, 7) and ld % 8 == 0 and ld < (1 << 20) and aligned:
        return f"im2col_nchw_stem_kernel<{S}, {D}, 3, 7, 7>"
    if not nchw and x_dtype == out_dtype and C % 8 == 0 and ld % 8 == 0 and ld == kh * kw * C and aligned:
        return f"im2col_nhwc_vec_kernel<{S}>"
    return f"im2col_kernel<{S}, {D}, {'true' if nchw else 'false'}>"


def col2im_route(dtype, C, ld, aligned, add=False):
    """the symbol dvt_col2im launches, or "unsupported" (the second path needs the vector route)"""
    T = CXX[dtype]
    if C % 8 == 0 and ld % 8 == 0 and aligned:
        return f"col2im_nhwc_kernel<{T}>"
    return "unsupported" if add else f"col2im_scalar_kernel<{T}, {T}, false>"


def col2im_nchw_route(dtype, dx_dtype):
    assert (dtype, dx_dtype) in PAIRS7
    return f"col2im_scalar_kernel<{CXX[dtype]}, {CXX[dx_dtype]}, true>"


def nhwc_pad_route(x_dtype, y_dtype, cpad):
    assert (x_dtype, y_dtype) in PAIRS6 and cpad in (4, 8)
    return f"nchw_to_nhwc_{'pad8' if cpad == 8 else 'pair4'}_kernel<{CXX[x_dtype]}, {CXX[y_dtype]}>"


def pack_plan(cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind, dtype, src_aligned=True, dst_aligned=True):
    """what one entry of the grouped pack runs: (form, rows per workgroup, workgroups, load branch, store branch) with form
    rows | tile | elems and branches "vec" | "scalar" (None where the form has none)"""
    taps = kh * kw
    rowlen = cin_l * taps
    load = "vec" if rowlen % 4 == 0 and src_aligned else "scalar"
    sixteen = dtype in ("bf16", "fp16")
    if kind == 0:
        if rowlen > PACK_ROW_MAX or ld > 4 * PACK_ROW_MAX:
            return "elems", 0, -(-cout_p * ld // 2048), None, None
        R = 1 if ld >= 2048 else 2048 // ld
        store = "vec" if sixteen and cin_p % 8 == 0 and ld % 8 == 0 and dst_aligned else "scalar"
        return "rows", R, -(-cout_p // R), load, store
    store = "vec" if sixteen and cout_p % 8 == 0 and dst_aligned else "scalar"
    return "tile", 0, -(-cout_p // 64) * -(-cin_p * taps // 64), load, store


def grid_cap(cus):
    """items one trip of a streaming kernel's grid covers when the grid is capped"""
    return GRID_BLOCKS_PER_CU * cus * BLOCK


def conv_hip_constants():
    """the constants the mirrors restate, read from conv.hip and common.h"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data-efficient-video-transformers_amd", "csrc")
    with open(os.path.join(root, "conv.hip")) as fh:
        conv = fh.read()
    with open(os.path.join(root, "common.h")) as fh:
        common = fh.read()
    return {"PACK_GROUP": int(re.search(r"constexpr int kPackGroup = (\d+);", conv).group(1)),
            "PACK_ROW_MAX": int(re.search(r"constexpr int kPackRowMax = (\d+);", conv).group(1)),
            "BLOCK": int(re.search(r"constexpr int kB = (\d+);", conv).group(1)),
            "GRID_BLOCKS_PER_CU": int(re.search(r"cap = \(int64_t\)dvt_num_cus\(\) \* (\d+);", common).group(1))}
