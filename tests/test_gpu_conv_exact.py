"""Exact results of every implicit-GEMM convolution kernel: the A_CONV forms of gemm_dma_kernel (forward / data gradient,
split-K slabs, weight gradient) and the reduces behind them (conv_split_reduce_kernel, splitk_reduce_conv_tiled_kernel, the
convolution-scatter mode of splitk_reduce_pending_kernel).

Each case states the plan it expects (ops.conv2d_implicit_plan: configuration, slices, K per slice, epilogue, output form,
reduce, carry) and checks it before launching; operands come from tests/conv_exact.py, so the output must equal the float64
reference -- torch.nn.functional.conv2d and its adjoints written out, never a kernel of this project -- bit for bit
(torch.equal).  Outputs are NaN inside and canary bits in spare rows behind, which must survive; the statistics buffer
likewise; operands sit in front of NaN-filled memory.  The launches go through the C ABI descriptor directly so that the
test owns every buffer.  tests/test_conv_coverage.py ties every kernel symbol of the family to one of these cases.

Not reachable through the ABI, hence without a case: the weight gradient on configuration 4 (conv_cfg puts every weight
gradient of at most 64 output channels on configuration 6); the gate lists it as unreachable and sweeps for it.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import conv_exact as V
from tests import gemm_exact as X

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
DTYPES = {"bf16": BF, "fp16": FP}
NONE, RES = 0, 3


def F(geom, cfg, kps, split=1, trim_w=0):
    N, Cc, H, W, Cout, k, stride, pad = geom
    return dict(N=N, C=Cc, H=H, W=W, Cout=Cout, k=k, stride=stride, pad=pad, trim_w=trim_w, cfg=cfg, split=split, kps=kps)


# Forward / stride-1 data gradient (the same launch on dz with rotated weights): N, C, H, W, Cout, k, stride, pad -> the
# configuration conv_fwd_cfg / conv_fwd_split give at 256 CUs.  Every case runs with statistics and with a residual.
FWD_CASES = {
    # 256 x 256 x 64: 51,072 rows (ragged last row tile), 144 columns (one ragged column tile)
    "f0_n144": F((16, 64, 56, 57, 144, 3, 1, 1), 0, 576),
    # 256 x 128 x 32: a k-tile inside one tap of 32 channels; 1,200 rows (ragged)
    "f1_c32": F((3, 32, 20, 20, 128, 3, 1, 1), 1, 288),
    # ... 288 columns (the width rule: 3 tiles of 128, the last 32 wide), C % 64 != 0, K = 864 -> 896
    "f1_n288": F((2, 96, 14, 14, 288, 3, 1, 1), 1, 896),
    # 256 x 64 x 32, the C == 8 stem form on the pixel-pair geometry: (7, 4) kernel, stride (2, 1), trim_w
    "f4_stem": F((2, 8, 32, 20, 64, (7, 4), (2, 1), (3, 2)), 4, 224, trim_w=1),
    # ... C % 32 != 0: taps split a k-tile, K = 216 -> 224; stride 2
    "f4_c24_s2": F((2, 24, 17, 13, 64, 3, 2, 1), 4, 224),
    # 256 x 64 x 64
    "f6_c64": F((3, 64, 20, 20, 64, 3, 1, 1), 6, 576),
    # ... taps that split a 64-deep k-tile (144 channels x 3 temporal taps = 432 -> 448); (3, 1) kernel
    "f6_c144_31": F((2, 144, 12, 49, 64, (3, 1), 1, (1, 0)), 6, 448),
    # 256 x 128 x 64: 24,640 rows (ragged), (1, 3) kernel
    "f7_13": F((8, 64, 56, 55, 256, (1, 3), 1, (0, 1)), 7, 192),
    # 128 x 128 x 64, two per CU
    "f9_n512": F((3, 64, 56, 56, 512, (1, 3), 1, (0, 1)), 9, 192),
    # 128 x 128 x 64, at most one per CU (the four-deep ring); 1,200 rows (ragged)
    "f10_n128": F((3, 64, 20, 20, 128, 3, 1, 1), 10, 576),
    # ... 1 x 1 stride 2
    "f10_1x1_s2": F((4, 64, 16, 16, 128, 1, 2, 0), 10, 64),
    # split-K slabs + conv_split_reduce_kernel: 45 k-tiles over 7 slices (uneven: the last slice has 3), two per CU
    "s9_uneven": F((8, 320, 14, 14, 512, 3, 1, 1), 9, 448, split=7),
    # ... 147 rows (a ragged row tile), 36 k-tiles over 6 slices, one per CU
    "s10_ragged": F((3, 256, 7, 7, 512, 3, 1, 1), 10, 384, split=6),
}


def W(geom, cfg, split, kps, scatter="scatter", logical=None, trim_w=0):
    d = F(geom, cfg, kps, split, trim_w)
    d.update(scatter=scatter, logical=logical)
    return d


# Weight gradient: configuration of conv_cfg(wgrad), slices of conv_wgrad_plan at 256 CUs.  Every case runs the packed
# result (plain reduce), the master-layout scatter with accumulate, the deferred + flushed reduce and the carried one.
WGRAD_CASES = {
    "w6_ragged": W((7, 64, 6, 6, 64, 3, 1, 1), 6, 1, 256),                   # 252 pixels on 64-deep k-tiles
    "w6_stem": W((2, 8, 32, 20, 64, (7, 4), (2, 1), (3, 2)), 6, 2, 320, trim_w=1),   # C == 8, 640 pixels = 10 k-tiles in 2 slices
    "w7_split4": W((4, 64, 16, 16, 128, 3, 1, 1), 7, 4, 256),
    "w7_padded": W((2, 24, 8, 8, 72, 3, 1, 1), 7, 1, 128, logical=(70, 21)),   # channel-padded layer: 70 x 21 of 72 x 24 exist
    "w7_31_s2": W((5, 128, 9, 5, 128, (3, 1), (2, 1), (1, 0)), 7, 1, 128),   # 125 pixels (ragged), strided temporal taps
    "w0_split3": W((6, 128, 12, 12, 256, 3, 1, 1), 0, 3, 320),               # 864 pixels: 13.5 k-tiles in 3 slices
    "w1_n288": W((5, 96, 9, 9, 288, 3, 1, 1), 1, 3, 160),                    # 405 pixels on 32-deep k-tiles (ragged)
    "w0_tiled": W((2, 264, 6, 6, 520, 3, 1, 1), 0, 1, 128, scatter="scatter_tiled"),   # 2,376 x 520 > 2^20 entries
}

# Strided data gradient by parity classes: N, Cin, H, W, Cout, k, stride, pad of the forward layer; shortcut gradient
# ("full": residual in full rows; "compact": residual_compact into class (0, 0)); configuration of every class launch.
DGRAD_CASES = {
    "d_3x3s2_full": dict(geom=(2, 64, 9, 11, 128, 3, 2, 1), short="full", cfg=6),
    "d_3x3s2_compact": dict(geom=(2, 128, 14, 14, 256, 3, 2, 1), short="compact", cfg=10),
    "d_31s21_none": dict(geom=(2, 64, 12, 49, 64, (3, 1), (2, 1), (1, 0)), short=None, cfg=6),
}


def stats_rows(name):
    """output rows behind one BatchNorm partial row: a wave row of the tile (128 in configurations 0 and 1, else 64), or
    the 64 rows of a workgroup of conv_split_reduce_kernel"""
    c = FWD_CASES[name]
    return 128 if c["split"] == 1 and c["cfg"] in (0, 1) else 64


def _ops():
    import dvt_amd
    return dvt_amd.ops, dvt_amd._lib


def _seed(c):
    return c["N"] * 7 + c["C"] * 3 + c["H"] * 11 + c["Cout"]


def expected_fwd_plan(name, residual, carry="none", carry_reduce="none"):
    from dvt_amd import ops
    c = FWD_CASES[name]
    split = c["split"] > 1
    return ops.ConvPlan(c["cfg"], c["split"], c["kps"], RES if residual and not split else NONE, "slab" if split else "map",
                        "split" if split else "none", False, carry, carry_reduce)


def fwd_plan(name, dtype, **kw):
    from dvt_amd import ops
    c = FWD_CASES[name]
    return ops.conv2d_implicit_plan(c["N"], c["C"], c["H"], c["W"], c["Cout"], c["k"], c["stride"], c["pad"], dtype,
                                    trim_w=c["trim_w"], **kw)


def expected_wgrad_plan(name, master, deferred):
    from dvt_amd import ops
    c = WGRAD_CASES[name]
    return ops.ConvPlan(c["cfg"], c["split"], c["kps"], NONE, "slab", c["scatter"] if master else "plain", deferred)


def wgrad_plan(name, dtype, **kw):
    from dvt_amd import ops
    c = WGRAD_CASES[name]
    return ops.conv2d_implicit_plan(c["N"], c["C"], c["H"], c["W"], c["Cout"], c["k"], c["stride"], c["pad"], dtype,
                                    wgrad=True, trim_w=c["trim_w"], **kw)


@functools.lru_cache(maxsize=2)
def build_fwd(name):
    """CPU float64: operands, packed weights, residual and the references of a forward case"""
    from dvt_amd import ops
    c = FWD_CASES[name]
    x, w = V.forward_operands(c["N"], c["C"], c["H"], c["W"], c["Cout"], c["k"], _seed(c))
    K = ops.conv2d_implicit_k(c["C"], c["Cout"], c["k"])
    y = V.conv_ref(x, w, c["stride"], c["pad"], c["trim_w"])
    res = X.small_ints(tuple(y.shape), -3, 3, _seed(c) + 5)
    return dict(x=x, w=w, wp=V.pack_weights(w, K), K=K, y=y, res=res, stats=V.stats_ref(y))


@functools.lru_cache(maxsize=2)
def build_wgrad(name):
    c = WGRAD_CASES[name]
    x, dz = V.wgrad_operands(c["N"], c["C"], c["H"], c["W"], c["Cout"], c["k"], c["stride"], c["pad"], _seed(c), c["trim_w"])
    dW = V.wgrad_ref(x, dz, c["k"], c["stride"], c["pad"])
    cout_l, cin_l = c["logical"] or (c["Cout"], c["C"])
    prior = X.small_ints((cout_l, cin_l) + tuple(dW.shape[2:]), -4, 4, _seed(c) + 9)
    return dict(x=x, dz=dz, dW=dW, prior=prior, cout_l=cout_l, cin_l=cin_l)


@functools.lru_cache(maxsize=2)
def build_dgrad(name):
    """dz sparse along its channels, w signed dense: the float64 input adjoint (+ the shortcut's gradient)"""
    c = DGRAD_CASES[name]
    N, Cin, H, Wd, Cout, k, stride, pad = c["geom"]
    (kh, kw), (sh, sw) = V.pair(k), V.pair(stride)
    Ho, Wo = V.out_hw(H, Wd, k, stride, pad)
    seed = N * 13 + Cin + H
    dz = V.sparse_map(N * Ho * Wo, Cout, seed).view(N, Ho, Wo, Cout)
    # (signs by (tap, output-channel range): the reduction of a class launch runs over its taps x Cout)
    w = V.signed_weights(Cin, Cout, kh, kw, seed + 1).permute(1, 0, 2, 3).contiguous()          # [Cout, Cin, kh, kw]
    dx = V.dgrad_ref(dz, w, H, Wd, stride, pad)
    out = dict(dz=dz, w=w, dx=dx, full=None, compact=None, Ho=Ho, Wo=Wo)
    if c["short"] == "full":
        out["full"] = X.small_ints(tuple(dx.shape), -3, 3, seed + 2)
        out["want"] = dx + out["full"]
    elif c["short"] == "compact":
        Hs, Ws = (H - 1) // sh + 1, (Wd - 1) // sw + 1
        out["compact"] = X.small_ints((N * Hs * Ws, Cin), -3, 3, seed + 2)
        want = dx.clone().view(N, H, Wd, Cin)
        want[:, ::sh, ::sw] += out["compact"].view(N, Hs, Ws, Cin)
        out["want"] = want.reshape(-1, Cin)
    else:
        out["want"] = dx
    return out


# ---------------------------------------------------------------- device buffers
def _guarded(t, dtype, device, tail=4096):
    """the values of `t` in front of NaN-filled memory: -> view of the buffer's first t.numel() elements, shaped like t"""
    buf = torch.full((t.numel() + tail,), float("nan"), dtype=dtype, device=device)
    view = buf[:t.numel()].view(t.shape)
    view.copy_(t.to(dtype))
    return view


def _desc(L, x, w, y, c, dtype, k=None, stride=None, pad=None, H=None, W=None, Cc=None, Cout=None, trim_w=None):
    from dvt_amd import ops
    (kh, kw), (sh, sw), (ph, pw) = V.pair(k or c["k"]), V.pair(stride or c["stride"]), V.pair(c["pad"] if pad is None else pad)
    d = L.ConvDesc()
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    d.N, d.H, d.W = c["N"], H or c["H"], W or c["W"]
    d.C, d.Cout = Cc or c["C"], Cout or c["Cout"]
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = kh, kw, sh, sw, ph, pw
    d.dtype = ops._DT[dtype]
    d.trim_w = c["trim_w"] if trim_w is None else trim_w
    return d


def _launch_fwd(ops, L, d, device):
    """dvt_conv2d_implicit on the test's own descriptor, with the workspace its size query asks for"""
    lib = L.load()
    need = int(lib.dvt_conv2d_implicit_workspace_bytes(C.byref(d)))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=device) if need else None
    if ws is not None:
        d.workspace = ws.data_ptr()
    L.check(lib.dvt_conv2d_implicit(C.byref(d), ops._stream()), "dvt_conv2d_implicit")
    torch.cuda.synchronize()
    return ws


def _stats_buffer(L, d, Cout, device):
    """-> (fp32 buffer [parts][2 * Cout] with canary bits in the rows behind -- the 64 that dvt_bn_stats_from_partials may
    fold into later, which the convolution must not touch, and 3 more --, parts)"""
    lib = L.load()
    parts = int(lib.dvt_conv2d_implicit_stats_parts(C.byref(d)))
    assert int(lib.dvt_conv2d_implicit_stats_bytes(C.byref(d))) == (parts + 64) * 2 * Cout * 4
    buf, _ = X.canaried(parts, 2 * Cout, torch.float32, device, pad=0, spare=67)
    return buf, parts


def run_forward(name, dtype, device, residual):
    """one launch of a forward case -> nothing; asserts the plan, the output, the canaries and the statistics"""
    ops, L = _ops()
    c = FWD_CASES[name]
    b = build_fwd(name)
    want = b["y"] + b["res"] if residual else b["y"]
    X.check_bound(want, dtype)
    assert fwd_plan(name, dtype, residual=residual, want_stats=not residual) == expected_fwd_plan(name, residual)
    x = _guarded(b["x"].reshape(-1, c["C"]), dtype, device)
    wp = _guarded(b["wp"], dtype, device)
    M, Cout = want.shape
    ybuf, y = X.canaried(M, Cout, dtype, device, pad=0, spare=3)
    d = _desc(L, x, wp, y, c, dtype)
    sbuf = parts = None
    if residual:
        r = _guarded(b["res"], dtype, device)
        d.residual = r.data_ptr()
    else:
        sbuf, parts = _stats_buffer(L, d, Cout, device)
        d.stats_partial = sbuf.data_ptr()
    _launch_fwd(ops, L, d, device)
    got = y.double().cpu()
    bad = int((got != want).sum()) + int(torch.isnan(got).sum())
    print(f"{name} {dtype} residual={residual}: {bad} of {want.numel()} outputs differ")
    assert torch.equal(got, want), f"{bad} outputs differ, first rows {sorted(set((got != want).nonzero()[:, 0].tolist()))[:8]}"
    assert X.canaries_intact(ybuf, M, Cout) == 0
    if sbuf is not None:
        V.check_stats_bound(want, stats_rows(name))
        part = sbuf[:parts].double().cpu().view(parts, 2, Cout)
        assert torch.equal(part.sum(0), b["stats"]), "the BatchNorm partial rows do not sum to the column sums / sums of squares"
        assert X.canaries_intact(sbuf, parts, 2 * Cout) == 0


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("residual", [False, True], ids=["stats", "res"])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_conv_forward_exact(device, name, residual, dname):
    run_forward(name, DTYPES[dname], device, residual)


# ---------------------------------------------------------------- strided data gradient by parity classes
def dgrad_classes(name):
    """-> [(a, b, taps (nth, ntw), pad', (rh, rw), (Hq, Wq))] of a case"""
    from dvt_amd import ops
    N, Cin, H, Wd, Cout, k, stride, pad = DGRAD_CASES[name]["geom"]
    return ops.strided_dgrad_classes(k, stride, pad, H, Wd)


def dgrad_class_plan(name, cls, dtype, residual, compact):
    from dvt_amd import ops
    N, Cin, H, Wd, Cout, k, stride, pad = DGRAD_CASES[name]["geom"]
    Ho, Wo = V.out_hw(H, Wd, k, stride, pad)
    (a, b, nt, pq, _, hq) = cls
    return ops.conv2d_implicit_plan(N, Cout, Ho, Wo, Cin, nt, 1, pq, dtype, out_hw=hq, out_rows=True, residual=residual,
                                    residual_compact=compact)


def class_rows(N, H, W, sh, sw, a, b):
    """the rows of the full-size map the pixels of parity class (a, b) name (written out here, not the library's table)"""
    n = torch.arange(N).view(-1, 1, 1)
    h = torch.arange(a, H, sh).view(1, -1, 1)
    w = torch.arange(b, W, sw).view(1, 1, -1)
    return (n * (H * W) + h * W + w).reshape(-1)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(DGRAD_CASES))
def test_conv_strided_dgrad_classes_exact(device, name, dname):
    ops, L = _ops()
    dtype = DTYPES[dname]
    c = DGRAD_CASES[name]
    N, Cin, H, Wd, Cout, k, stride, pad = c["geom"]
    (kh, kw), (sh, sw) = V.pair(k), V.pair(stride)
    b = build_dgrad(name)
    X.check_bound(b["want"], dtype)
    classes = dgrad_classes(name)
    assert classes is not None and len(classes) == sh * sw
    # every row of the result is written exactly once across the classes
    rows = [class_rows(N, H, Wd, sh, sw, a_, b_) for (a_, b_, *_rest) in classes]
    assert torch.equal(torch.cat(rows).sort().values, torch.arange(N * H * Wd))
    dz = _guarded(b["dz"].reshape(-1, Cout), dtype, device)
    wm = b["w"].float().to(device)
    M = N * H * Wd
    dxbuf, dx = X.canaried(M, Cin, dtype, device, pad=0, spare=3)
    full = _guarded(b["full"], dtype, device) if b["full"] is not None else None
    compact = _guarded(b["compact"], dtype, device) if b["compact"] is not None else None
    wcs, entries = [], []
    for (a_, b_, nt, pq, (rh, rw), hq) in classes:                   # kind 2: the class's taps, decreasing, channels transposed
        wc = _guarded(torch.zeros(Cin, nt[0] * nt[1] * Cout), dtype, device)
        entries.append((wm, wc, Cout, Cin, kh, kw, Cout, Cin, 0, 2, (sh, sw, rh, rw)))
        wcs.append(wc)
    ops.conv_weight_pack_group(entries)
    fake = dict(N=N, C=Cout, H=b["Ho"], W=b["Wo"], Cout=Cin, trim_w=0)
    for cls, wc, r in zip(classes, wcs, rows):
        (a_, b_, nt, pq, _, hq) = cls
        res, rc = (full, False) if full is not None else ((compact, True) if compact is not None and (a_, b_) == (0, 0) else (None, False))
        plan = dgrad_class_plan(name, cls, dtype, res is not None, rc)
        assert plan == ops.ConvPlan(c["cfg"], 1, nt[0] * nt[1] * Cout, RES if res is not None else NONE), (cls, plan)
        rows_dev = r.to(torch.int32).to(device)
        d = _desc(L, dz, wc, dx, fake, dtype, k=nt, stride=1, pad=pq)
        d.out_h, d.out_w = hq
        d.out_rows, d.residual_compact = rows_dev.data_ptr(), int(rc)
        if res is not None:
            d.residual = res.data_ptr()
        _launch_fwd(ops, L, d, device)
    got = dx.double().cpu()
    bad = int((got != b["want"]).sum()) + int(torch.isnan(got).sum())
    print(f"{name} {dtype}: {bad} of {got.numel()} outputs differ")
    assert torch.equal(got, b["want"])
    assert X.canaries_intact(dxbuf, M, Cin) == 0


# ---------------------------------------------------------------- weight gradient
def _launch_wgrad(ops, L, d, device, pending=None):
    lib = L.load()
    need = int(lib.dvt_conv2d_implicit_wgrad_workspace_bytes(C.byref(d)))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=device)
    d.workspace = ws.data_ptr()
    if pending is not None:
        d.defer_reduce, d.pending = 1, C.pointer(pending)
    L.check(lib.dvt_conv2d_implicit_wgrad(C.byref(d), ops._stream()), "dvt_conv2d_implicit_wgrad")
    torch.cuda.synchronize()
    return ws


def _master(b, device):
    """the parameter's gradient [cout_l][cin_l][kh][kw] holding `prior`, canary bits around it -> (buffer, flat view)"""
    n = b["prior"].numel()
    return X.canaried(1, n, torch.float32, device, pad=8, spare=1, fill=b["prior"].reshape(1, n))


# the launch that carries a deferred weight-gradient reduce: one slice -> in its grid tail; split -> launched alone first
CARRIERS = {"tail": "f10_1x1_s2", "alone": "s10_ragged"}


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_conv_wgrad_exact(device, name, dname):
    ops, L = _ops()
    dtype = DTYPES[dname]
    c = WGRAD_CASES[name]
    b = build_wgrad(name)
    kh, kw = V.pair(c["k"])
    Cc, Cout, cout_l, cin_l = c["C"], c["Cout"], b["cout_l"], b["cin_l"]
    dW = b["dW"]
    assert float(dW.abs().max()) + 4 < 2 ** 24
    x = _guarded(b["x"].reshape(-1, Cc), dtype, device)
    dz = _guarded(b["dz"].reshape(-1, Cout), dtype, device)
    # 1. the packed dWt [kh * kw * C, Cout] behind the plain reduce
    assert wgrad_plan(name, dtype) == expected_wgrad_plan(name, False, False)
    K = kh * kw * Cc
    tbuf, t = X.canaried(K, Cout, torch.float32, device, pad=0, spare=3)
    _launch_wgrad(ops, L, _desc(L, x, dz, t, c, dtype), device)
    want_t = dW.permute(2, 3, 1, 0).reshape(K, Cout)
    got = t.double().cpu()
    print(f"{name} {dtype} packed: {int((got != want_t).sum())} of {got.numel()} entries differ")
    assert torch.equal(got, want_t) and X.canaries_intact(tbuf, K, Cout) == 0
    # 2. - 4. the master-layout scatter with accumulate, of the channels the parameter has: alone, deferred + flushed,
    # deferred + carried in the grid tail of a forward launch / launched alone in front of a split one
    want_m = (b["prior"] + dW[:cout_l, :cin_l]).reshape(1, -1)
    kw_m = dict(master=True, accumulate=True, logical=c["logical"])
    for how in ("alone", "flushed", "carried"):
        assert wgrad_plan(name, dtype, defer_reduce=how != "alone", **kw_m) == expected_wgrad_plan(name, True, how != "alone")
        mbuf, m = _master(b, device)
        d = _desc(L, x, dz, m, c, dtype)
        d.wgrad_master_layout, d.wgrad_accumulate = 1, 1
        d.wgrad_cout_l, d.wgrad_cin_l = c["logical"] or (0, 0)
        pend = L.SplitKPending() if how != "alone" else None
        ws = _launch_wgrad(ops, L, d, device, pend)
        if how == "flushed":
            assert pend.valid
            ops.splitk_reduce_pending(pend)
        elif how == "carried":
            form = "alone" if c["scatter"] == "scatter_tiled" else "tail"       # (the large reduce goes in front of a split launch)
            carrier = CARRIERS[form]
            cc, cb = FWD_CASES[carrier], build_fwd(carrier)
            assert fwd_plan(carrier, dtype, carry=pend) == expected_fwd_plan(carrier, False, form, c["scatter"] if form == "alone" else "none")
            cx, cw = _guarded(cb["x"].reshape(-1, cc["C"]), dtype, device), _guarded(cb["wp"], dtype, device)
            cybuf, cy = X.canaried(cb["y"].shape[0], cc["Cout"], dtype, device, pad=0, spare=3)
            cd = _desc(L, cx, cw, cy, cc, dtype)
            cd.carry = C.pointer(pend)
            _launch_fwd(ops, L, cd, device)
            assert torch.equal(cy.double().cpu(), cb["y"]) and X.canaries_intact(cybuf, cb["y"].shape[0], cc["Cout"]) == 0
        torch.cuda.synchronize()
        got = m.double().cpu()
        print(f"{name} {dtype} master {how}: {int((got != want_m).sum())} of {got.numel()} entries differ")
        assert torch.equal(got, want_m), how
        assert X.canaries_intact(mbuf, 1, want_m.numel()) == 0, how
        del ws
