"""Every LayerNorm kernel (csrc/layernorm.hip, csrc/ln_reduce.h) and the cross-entropy on integer labels (csrc/losses.hip)
called directly through ops.*, each output judged elementwise against the float64 statement of tests/layernorm_ref.py under
the rule of tests/rowwise_ref.py (4 x the fp32 chain's own error plus one fp32 ulp; a 16-bit output is the float64 result
rounded to the dtype or a neighbouring value), at the smallest shapes that reach each path: every VPL boundary and partly
filled last vector group, part / whole / one-more-than-whole workgroups, both reduce kernels and their unrolled loops, both
grid caps and their second grid-stride trip, every element-type combination the dispatch accepts.

Operands are rounded to the kernel's dtype before the reference and the kernel see them; the backward is handed the
float64 reference's mean / rstd rounded to fp32.  Outputs ops allocates sit in the NaN bands of ``guarded``; destinations
the caller owns come from ``poisoned`` (tests/guards.py).  tests/test_layernorm_coverage.py ties every kernel symbol of the
built library to a parameter set of this file."""
import ctypes as C
import math

import pytest
import torch

from tests import layernorm_ref as LR
from tests import rowwise_ref as R
from tests.guards import guarded, poisoned

pytestmark = pytest.mark.gpu

DT = ["fp32", "bf16", "fp16"]
# VPL = cdiv(d, 512), 5..8 -> 8: each VPL's smallest and largest d; 504 / 520 / 1032 / 1544 / 2056 leave the last lane group
# partly filled; 2 * 8 and 2 * 40 are no multiples of 32, so one reduce workgroup straddles dgamma | dbeta
WIDTHS = [8, 40, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4096]
ROWS = [1, 3, 4, 5, 9]                        # four waves per workgroup: a part workgroup, a whole one, one more than whole
FWD_TYPES = [("fp32", "fp32"), ("bf16", "bf16"), ("fp16", "fp16"), ("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "fp32"),
             ("fp16", "fp32")]                # (x, y)
# (dy, x, dx, dx_lp): the three equal triples; 16-bit dy into an fp32 stream without and with its 16-bit copy; fp32 dy into
# 16-bit rows
BWD_TYPES = [("fp32", "fp32", "fp32", None), ("bf16", "bf16", "bf16", None), ("fp16", "fp16", "fp16", None),
             ("bf16", "fp32", "fp32", None), ("fp16", "fp32", "fp32", None), ("bf16", "fp32", "fp32", "bf16"),
             ("fp16", "fp32", "fp32", "fp16"), ("fp32", "bf16", "bf16", None), ("fp32", "fp16", "fp16", None)]
# nparts = cdiv(rows, 4).  25 and 33 partial rows: either side of the end of the 4-way unrolled loop of
# ln_bwd_reduce_kernel<8> (p + 24 < nparts); 128 / 129: the switch from <8> to <32>; 1024 workgroups at 4096 rows is the
# backward's cap, the 4097th row is a second grid-stride trip of one wave
BWD_ROW_COUNTS = [100, 132, 512, 513, 4096, 4097]


def _ids(types):
    return ["-".join(("lp" if i == 3 else t) for i, t in enumerate(ts) if t is not None) for ts in types]


@pytest.fixture(scope="module")
def dvt(device):
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _cu_count(dvt):
    """the compute-unit count the library sizes its grids by"""
    n = C.c_int(0)
    dvt._lib.check(dvt._lib.load().dvt_device_info(C.byref(n), None, None, 0), "dvt_device_info")
    assert n.value > 0
    return n.value


def _x(shape, name, g):
    return LR.randn(shape, R.DTYPES[name], g, 1.5, 0.5)


def _fwd_dense(ops, device, x, gamma, beta, ydt, tag):
    """dense forward into outputs of ops' own, inside guard bands; judged on the CPU"""
    with guarded(ops):
        y, mean, rstd = ops.layernorm_fwd(x.to(device), gamma.to(device), beta.to(device), LR.EPS, out_dtype=ydt)
    assert y.dtype == ydt and y.shape == x.shape
    LR.check_fwd(y.cpu(), mean.cpu(), rstd.cpu(), x, gamma, beta, tag)


def _bwd_dense(ops, device, dy, x, gamma, beta, dxt, lp, tag, **extra):
    """dense backward into outputs of ops' own; ``extra``: dx_add"""
    mean, rstd = LR.stats32(x, gamma, beta)
    dev = {k: v.to(device) for k, v in extra.items()}
    with guarded(ops):
        out = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                                dx_dtype=dxt, dx_lp=lp, **dev)
    assert out[0].dtype == dxt and len(out) == (3 if lp is None else 4)
    LR.check_bwd(out[0].cpu(), out[1].cpu(), out[2].cpu(), dy, x, gamma, mean, rstd, tag, dx_add=extra.get("dx_add"),
                 dx_lp=None if lp is None else out[3].cpu())


# ---------------------------------------------------------------- every instantiation: widths x types x row counts
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("types", FWD_TYPES, ids=_ids(FWD_TYPES))
def test_ln_fwd(dvt, device, types, d):
    xn, yn = types
    g = LR.gen(1000 + d)
    gamma, beta = LR.ln_params(d, g)
    for rows in ROWS:
        _fwd_dense(dvt.ops, device, _x((rows, d), xn, g), gamma, beta, R.DTYPES[yn], f"{xn}->{yn} rows={rows} d={d}")


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("types", BWD_TYPES, ids=_ids(BWD_TYPES))
def test_ln_bwd(dvt, device, types, d):
    dyn, xn, dxn, lpn = types
    g = LR.gen(2000 + d)
    gamma, beta = LR.ln_params(d, g)
    for rows in ROWS:
        x = _x((rows, d), xn, g)
        dy = LR.randn((rows, d), R.DTYPES[dyn], g)
        _bwd_dense(dvt.ops, device, dy, x, gamma, beta, R.DTYPES[dxn], None if lpn is None else R.DTYPES[lpn],
                   f"{dyn},{xn}->{dxn}{'+lp' if lpn else ''} rows={rows} d={d}")


# ---------------------------------------------------------------- row counts: the reduce kernels and the grid caps
@pytest.mark.parametrize("rows", BWD_ROW_COUNTS)
def test_ln_bwd_row_counts(dvt, device, rows):
    d = 8
    for name in ("fp32", "bf16"):
        g = LR.gen(3000 + rows)
        gamma, beta = LR.ln_params(d, g)
        x = _x((rows, d), name, g)
        dy = LR.randn((rows, d), R.DTYPES[name], g)
        _fwd_dense(dvt.ops, device, x, gamma, beta, R.DTYPES[name], f"{name} rows={rows} d={d}")
        _bwd_dense(dvt.ops, device, dy, x, gamma, beta, R.DTYPES[name], None, f"{name} rows={rows} d={d}",
                   dx_add=LR.randn((rows, d), R.DTYPES[name], g))


@pytest.mark.parametrize("more", [0, 3])
def test_ln_fwd_grid_cap(dvt, device, more):
    """the forward launches at most 8 workgroups of four waves per compute unit: 4 * 8 * CUs rows fill that grid once, three
    rows more send three waves of the first workgroup on a second trip"""
    d = 8
    rows = 4 * 8 * _cu_count(dvt) + more
    for xn, yn in (("fp32", "fp32"), ("fp16", "fp16"), ("bf16", "fp32")):
        g = LR.gen(4000 + more)
        gamma, beta = LR.ln_params(d, g)
        _fwd_dense(dvt.ops, device, _x((rows, d), xn, g), gamma, beta, R.DTYPES[yn], f"{xn}->{yn} rows={rows} d={d}")


# ---------------------------------------------------------------- strided rows
def _pitched(t, pitch, dtype, device, fill=math.nan):
    """[n0, n1, d] CPU -> (device buffer [n0, n1, pitch] inside guard bands whose [..., :d] holds t, its check): the pitch
    padding is ``fill``"""
    n0, n1, d = t.shape
    buf, check = poisoned((n0, n1, pitch), dtype, device, fill=fill)
    buf[..., :d] = t.to(device)
    return buf, check


@pytest.mark.parametrize("d", [8, 520])
@pytest.mark.parametrize("name", DT)
def test_ln_strided_rows(dvt, device, name, d):
    """(n0, n1) = (3, 5): x rows at a pitch of d + 8, y / dy rows at a pitch of d + 16 (out_rows / dy_rows); dx goes by x's
    strides.  The padding between the rows is poisoned: NaN in the inputs (a read of it would reach an output), a sentinel
    in the outputs that must still be there."""
    dtype, ops = R.DTYPES[name], dvt.ops
    n0, n1, px, py = 3, 5, d + 8, d + 16
    g = LR.gen(5000 + d)
    gamma, beta = LR.ln_params(d, g)
    x = _x((n0, n1, d), name, g)
    dy = LR.randn((n0, n1, d), dtype, g)
    x2, dy2 = x.view(-1, d), dy.view(-1, d)
    tag = f"{name} strided d={d}"
    xb, chk_x = _pitched(x, px, dtype, device)
    yb, chk_y = poisoned((n0, n1, py), dtype, device, fill=-7.0)
    with guarded(ops):                                                        # (mean / rstd are ops' own)
        y, mean, rstd = ops.layernorm_fwd(xb[..., :d], gamma.to(device), beta.to(device), LR.EPS, rows=(n0, n1, n1 * px, px),
                                          out=yb, out_rows=(n1 * py, py))
    chk_x(); chk_y()
    assert y is yb and bool((yb[..., d:] == -7.0).all()), "y's pitch padding was written"
    LR.check_fwd(yb[..., :d].cpu().reshape(-1, d), mean.cpu(), rstd.cpu(), x2, gamma, beta, tag)

    mean, rstd = LR.stats32(x2, gamma, beta)
    dyb, chk_dy = _pitched(dy, py, dtype, device)
    dxb, chk_dx = poisoned((n0, n1, px), dtype, device, fill=-7.0)
    dg, chk_g = poisoned((d,), torch.float32, device)
    db, chk_b = poisoned((d,), torch.float32, device)
    out = ops.layernorm_bwd(dyb[..., :d], xb[..., :d], gamma.to(device), mean.to(device), rstd.to(device),
                            rows=(n0, n1, n1 * px, px), dy_rows=(n1 * py, py), dx=dxb, dg=dg, db=db)
    for c in (chk_x, chk_dy, chk_dx, chk_g, chk_b):
        c()
    assert out[0] is dxb and bool((dxb[..., d:] == -7.0).all()), "dx's pitch padding was written"
    LR.check_bwd(dxb[..., :d].cpu().reshape(-1, d), dg.cpu(), db.cpu(), dy2, x2, gamma, mean, rstd, tag)


@pytest.mark.parametrize("name", DT)
def test_ln_cls_rows(dvt, device, name):
    """rows = (n0, 1, n1 d, 0): row 0 of every group of n1 rows of a dense x; y and dy are dense [n0, d] (dy_rows (d, 0)),
    dx is written at x's offsets and the other n1 - 1 rows of every group keep their sentinel"""
    dtype, ops = R.DTYPES[name], dvt.ops
    n0, n1 = 3, 5
    for d in (40, 1032):
        g = LR.gen(5500 + d)
        gamma, beta = LR.ln_params(d, g)
        x = _x((n0, n1, d), name, g)
        x0 = x[:, 0].contiguous()
        dy = LR.randn((n0, d), dtype, g)
        tag = f"{name} cls rows d={d}"
        with guarded(ops):
            y, mean, rstd = ops.layernorm_fwd(x.to(device), gamma.to(device), beta.to(device), LR.EPS, rows=(n0, 1, n1 * d, 0))
        assert y.shape == (n0, d)
        LR.check_fwd(y.cpu(), mean.cpu(), rstd.cpu(), x0, gamma, beta, tag)
        mean, rstd = LR.stats32(x0, gamma, beta)
        dxb, chk_dx = poisoned((n0, n1, d), dtype, device, fill=-7.0)
        with guarded(ops):                                                    # (dgamma / dbeta are ops' own)
            _, dg, db = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                                          rows=(n0, 1, n1 * d, 0), dy_rows=(d, 0), dx=dxb)
        chk_dx()
        assert bool((dxb[:, 1:] == -7.0).all()), "dx rows outside the selection were written"
        LR.check_bwd(dxb[:, 0].cpu(), dg.cpu(), db.cpu(), dy, x0, gamma, mean, rstd, tag)


# ---------------------------------------------------------------- first-row operands, dx_add, aliasing
@pytest.mark.parametrize("types", BWD_TYPES[:5] + BWD_TYPES[7:], ids=_ids(BWD_TYPES[:5] + BWD_TYPES[7:]))
def test_ln_first_row_operands(dvt, device, types):
    """dy_first (dy's type) and dx_first (dx's type), each [n0, d] at a row stride of its own, with dx_add: dy_first enters
    dgamma / dbeta, the other two enter dx only"""
    dyn, xn, dxn, _ = types
    ops, n0, n1 = dvt.ops, 3, 5
    for d in (40, 520):
        g = LR.gen(6000 + d)
        gamma, beta = LR.ln_params(d, g)
        x = _x((n0 * n1, d), xn, g)
        dy = LR.randn((n0 * n1, d), R.DTYPES[dyn], g)
        add = LR.randn((n0 * n1, d), R.DTYPES[dxn], g)
        dyf = LR.randn((n0, d), R.DTYPES[dyn], g)
        dxf = LR.randn((n0, d), R.DTYPES[dxn], g, 2.0)
        dyf_b, chk1 = _pitched(dyf.unsqueeze(0), d + 8, R.DTYPES[dyn], device)      # [1, n0, d + 8]
        dxf_b, chk2 = _pitched(dxf.unsqueeze(0), d + 24, R.DTYPES[dxn], device)
        mean, rstd = LR.stats32(x, gamma, beta)
        with guarded(ops):
            dx, dg, db = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                                           rows=(n0, n1, n1 * d, d), dx_add=add.to(device), dy_first=dyf_b[0, :, :d],
                                           dx_first=dxf_b[0, :, :d], dx_dtype=R.DTYPES[dxn])
        chk1(); chk2()
        LR.check_bwd(dx.cpu(), dg.cpu(), db.cpu(), dy, x, gamma, mean, rstd, f"{dyn},{xn}->{dxn} first rows d={d}",
                     dx_add=add, dy_first=dyf, dx_first=dxf, n1=n1)


@pytest.mark.parametrize("name", DT)
def test_ln_dx_add_aliases_dx(dvt, device, name):
    """dx_add is dx itself: every element is read by the lane that then writes it, which is why the kernel's dx_add and dx
    pointers are not __restrict__.  functional.py relies on it: the folded CLS attention backward adds the query path's
    LayerNorm gradient into the rows of dx that attn_cls_bwd has just written (dx=dxf, dx_add=dxf, on the CLS rows)."""
    dtype, ops = R.DTYPES[name], dvt.ops
    n0, n1 = 3, 5
    for d in (8, 1544):
        g = LR.gen(6500 + d)
        gamma, beta = LR.ln_params(d, g)
        x = _x((n0, n1, d), name, g)
        x0 = x[:, 0].contiguous()
        dy = LR.randn((n0, d), dtype, g)
        old = LR.randn((n0, n1, d), dtype, g)
        dxf = LR.randn((n0, d), dtype, g)
        mean, rstd = LR.stats32(x0, gamma, beta)
        dxb, chk = poisoned((n0, n1, d), dtype, device)
        dxb.copy_(old.to(device))
        dg0, db0 = torch.randn(d, generator=g), torch.randn(d, generator=g)
        dg, chk_g = poisoned((d,), torch.float32, device)
        db, chk_b = poisoned((d,), torch.float32, device)
        dg.copy_(dg0.to(device)); db.copy_(db0.to(device))
        ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                          rows=(n0, 1, n1 * d, 0), dy_rows=(d, 0), dx=dxb, dx_add=dxb, dx_first=dxf.to(device), dg=dg, db=db,
                          accumulate=True)                                    # (the call of functional.py, as it stands there)
        chk(); chk_g(); chk_b()
        assert torch.equal(dxb[:, 1:].cpu(), old[:, 1:]), "dx rows outside the selection changed"
        LR.check_bwd(dxb[:, 0].cpu(), dg.cpu(), db.cpu(), dy, x0, gamma, mean, rstd, f"{name} aliased d={d}",
                     dx_add=old[:, 0].contiguous(), dx_first=dxf, dg0=dg0, db0=db0)


@pytest.mark.parametrize("acc_b", [False, True])
@pytest.mark.parametrize("acc_g", [False, True])
def test_ln_accumulate(dvt, device, acc_g, acc_b):
    """accumulate / accumulate_beta separately, onto non-zero dg / db; a destination that is overwritten starts as NaN"""
    ops = dvt.ops
    for name, rows, d in (("fp32", 9, 40), ("bf16", 513, 8), ("fp16", 5, 520)):
        dtype = R.DTYPES[name]
        g = LR.gen(7000 + d)
        gamma, beta = LR.ln_params(d, g)
        x = _x((rows, d), name, g)
        dy = LR.randn((rows, d), dtype, g)
        mean, rstd = LR.stats32(x, gamma, beta)
        dg0, db0 = 3.0 * torch.randn(d, generator=g), 3.0 * torch.randn(d, generator=g)
        dg, chk_g = poisoned((d,), torch.float32, device)
        db, chk_b = poisoned((d,), torch.float32, device)
        if acc_g:
            dg.copy_(dg0.to(device))
        if acc_b:
            db.copy_(db0.to(device))
        with guarded(ops):                                                    # (dx is ops' own)
            dx, dg_o, db_o = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                                               dg=dg, db=db, accumulate=acc_g, accumulate_beta=acc_b)
        chk_g(); chk_b()
        assert dg_o is dg and db_o is db
        LR.check_bwd(dx.cpu(), dg.cpu(), db.cpu(), dy, x, gamma, mean, rstd, f"{name} acc={acc_g},{acc_b} rows={rows} d={d}",
                     dg0=dg0 if acc_g else None, db0=db0 if acc_b else None)


# ---------------------------------------------------------------- the deferred reduce
# (rows, d, accumulate, accumulate_beta): the group grid is sized for the widest entry (d = 1032: 65 column blocks), the
# narrower ones return early on most of it; 132 and 516 rows give 33 and 129 partial rows
DEFERRED = [(9, 520, False, False), (5, 8, True, False), (132, 40, False, True), (3, 8, True, True), (4, 1032, False, False),
            (516, 8, True, True)]


def test_ln_deferred_reduce(dvt, device):
    """several layernorm_bwd(defer=...) of different widths and accumulate bits, one layernorm_flush(): dx is final at
    once, dg / db only after the flush, and every callback is seen once, in order"""
    ops = dvt.ops
    ops.layernorm_flush()
    assert not ops._ln_deferred
    seen, cases = [], []
    for k, (rows, d, acc_g, acc_b) in enumerate(DEFERRED):
        g = LR.gen(8000 + k)
        gamma, beta = LR.ln_params(d, g)
        x = _x((rows, d), "fp32", g)
        dy = LR.randn((rows, d), torch.float32, g)
        mean, rstd = LR.stats32(x, gamma, beta)
        dg0, db0 = torch.randn(d, generator=g) + 2.0, torch.randn(d, generator=g) - 2.0
        dg, chk_g = poisoned((d,), torch.float32, device)
        db, chk_b = poisoned((d,), torch.float32, device)
        if acc_g:
            dg.copy_(dg0.to(device))
        if acc_b:
            db.copy_(db0.to(device))
        before = (dg.cpu().clone(), db.cpu().clone())
        with guarded(ops):
            dx, _, _ = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device),
                                         dg=dg, db=db, accumulate=acc_g, accumulate_beta=acc_b,
                                         defer=lambda k=k: seen.append(k))
        cases.append((dx, dg, db, chk_g, chk_b, before, dy, x, gamma, mean, rstd, dg0 if acc_g else None, db0 if acc_b else None))
    with guarded(ops):                                                        # no callback, destinations of ops' own
        g = LR.gen(8100)
        gamma, beta = LR.ln_params(72, g)
        x, dy = _x((7, 72), "bf16", g), LR.randn((7, 72), torch.bfloat16, g)
        mean, rstd = LR.stats32(x, gamma, beta)
        own = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device), defer=True)
        own_operands = (dy, x, gamma, mean, rstd)
        assert seen == [] and len(ops._ln_deferred) == len(DEFERRED) + 1
        for dx, dg, db, _, _, before, *_ in cases:                            # nothing has reached dg / db yet
            assert torch.equal(dg.cpu().nan_to_num(nan=-1.0), before[0].nan_to_num(nan=-1.0))
            assert torch.equal(db.cpu().nan_to_num(nan=-1.0), before[1].nan_to_num(nan=-1.0))
        ops.layernorm_flush()
        torch.cuda.synchronize()
    assert seen == list(range(len(DEFERRED))) and not ops._ln_deferred
    for k, (dx, dg, db, chk_g, chk_b, _, dy, x, gamma, mean, rstd, dg0, db0) in enumerate(cases):
        chk_g(); chk_b()
        LR.check_bwd(dx.cpu(), dg.cpu(), db.cpu(), dy, x, gamma, mean, rstd, f"deferred entry {k} {DEFERRED[k]}", dg0=dg0, db0=db0)
    LR.check_bwd(own[0].cpu(), own[1].cpu(), own[2].cpu(), *own_operands, "deferred entry of ops' own")
    ops.layernorm_flush()                                                     # an empty list: nothing happens
    assert seen == list(range(len(DEFERRED)))


@pytest.mark.parametrize("count", [33, 34])
def test_ln_reduce_group_direct(dvt, device, count):
    """dvt_layernorm_reduce_group on a list longer than one launch takes (32), with one valid = 0 entry early in it -- ops
    never gets there, it flushes at 24 entries.  33 entries: 32 valid ones, which one launch takes; 34: the 33rd valid entry
    is a second launch.  The skipped entry's destinations keep their sentinel; the last entries accumulate, so an entry
    reduced twice shows."""
    L = dvt._lib
    skip, entries = 5, []
    arr = (L.LnPending * count)()
    for i in range(count):
        d = (8, 40, 72)[i % 3]
        nparts = (1, 25, 33, 130, 7)[i % 5]                                   # 130: the 4-way unrolled loop at PL = 32 and its tail
        g = LR.gen(9000 + i)
        part = torch.randn(nparts, 2, d, generator=g)
        acc = 3 if i >= count - 2 else i % 4
        dg0, db0 = torch.randn(d, generator=g) + 1.0, torch.randn(d, generator=g) - 1.0
        keep = i == skip
        dg, chk_g = poisoned((d,), torch.float32, device, fill=-7.0 if keep else math.nan)
        db, chk_b = poisoned((d,), torch.float32, device, fill=-7.0 if keep else math.nan)
        if acc & 1 and not keep:
            dg.copy_(dg0.to(device))
        if acc & 2 and not keep:
            db.copy_(db0.to(device))
        part_d = part.to(device)
        e = arr[i]
        e.partial, e.nparts, e.d, e.dgamma, e.dbeta = part_d.data_ptr(), nparts, d, dg.data_ptr(), db.data_ptr()
        e.accumulate, e.valid = acc, 0 if keep else 1
        entries.append((part, part_d, dg, db, chk_g, chk_b, dg0 if acc & 1 else None, db0 if acc & 2 else None))
    torch.cuda.synchronize()
    L.check(L.load().dvt_layernorm_reduce_group(arr, count, dvt.ops._stream()), "dvt_layernorm_reduce_group")
    torch.cuda.synchronize()
    for i, (part, _, dg, db, chk_g, chk_b, dg0, db0) in enumerate(entries):
        chk_g(); chk_b()
        if i == skip:
            assert bool((dg == -7.0).all()) and bool((db == -7.0).all()), "an entry with valid = 0 was reduced"
            continue
        for got, col, base, what in ((dg, 0, dg0, "dgamma"), (db, 1, db0, "dbeta")):
            p = part[:, col]
            b64 = 0.0 if base is None else base.double()
            b32 = 0.0 if base is None else base
            mag = p.double().abs().max(0).values if base is None else torch.maximum(p.double().abs().max(0).values, base.double().abs())
            R.assert_close(got.cpu(), p.double().sum(0) + b64, p.sum(0) + b32, mag, f"group {what} entry {i} of {count}")


# ---------------------------------------------------------------- input content
@pytest.mark.parametrize("name", DT)
def test_ln_offset_rows(dvt, device, name):
    """rows of mean 100 and spread 0.1: the two-pass variance keeps what E[x^2] - E[x]^2 would lose entirely"""
    dtype = R.DTYPES[name]
    for d in (8, 520, 4096):
        g = LR.gen(10000 + d)
        gamma, beta = LR.ln_params(d, g)
        x = LR.offset_rows(9, d, dtype, g)
        _fwd_dense(dvt.ops, device, x, gamma, beta, dtype, f"{name} offset rows d={d}")
        _bwd_dense(dvt.ops, device, LR.randn((9, d), dtype, g), x, gamma, beta, dtype, None, f"{name} offset rows d={d}")


@pytest.mark.parametrize("name", DT)
def test_ln_constant_row(dvt, device, name):
    """a constant row among ordinary ones: its variance is exactly 0, rstd = 1 / sqrt(eps), y = beta and dx is rstd times
    the centred g.  The constant row is judged on its own, so that it and the ordinary rows do not share a budget.
    d is a power of two here: then sum / d is exact in any fp32 evaluation and the row's centred values are exactly zero.
    At another d the product sum * fl(1 / d) may miss the constant by an ulp, which rstd = 316 turns into 1e-4 of y, while
    the CPU chain's sum / d happens to be exact and would leave a budget of one ulp -- a statement about that row of
    inputs, not about the kernel (the offset rows above cover a mean rounded at such a d)."""
    dtype, ops = R.DTYPES[name], dvt.ops
    for d in (8, 1024):
        g = LR.gen(11000 + d)
        gamma, beta = LR.ln_params(d, g)
        x = _x((5, d), name, g)
        x[3] = LR.constant_rows(1, d, dtype)[0]
        dy = LR.randn((5, d), dtype, g)
        mean, rstd = LR.stats32(x, gamma, beta)
        assert float(rstd[3]) == float((1.0 / torch.sqrt(torch.tensor(LR.EPS, dtype=torch.float64))).float())
        with guarded(ops):
            y, m, r = ops.layernorm_fwd(x.to(device), gamma.to(device), beta.to(device), LR.EPS)
        with guarded(ops):
            dx, dg, db = ops.layernorm_bwd(dy.to(device), x.to(device), gamma.to(device), mean.to(device), rstd.to(device))
        y, m, r, dx = y.cpu(), m.cpu(), r.cpu(), dx.cpu()
        for sel, what in (([3], "the constant row"), ([0, 1, 2, 4], "the other rows")):
            tag = f"{name} {what} d={d}"
            LR.check_fwd(y[sel], m[sel], r[sel], x[sel], gamma, beta, tag)
            LR.check_bwd(dx[sel], None, None, dy[sel], x[sel], gamma, mean[sel], rstd[sel], tag)
        assert torch.equal(y[3].float(), beta.to(dtype).float())
        LR.check_bwd(None, dg.cpu(), db.cpu(), dy, x, gamma, mean, rstd, f"{name} with a constant row d={d}")


def test_ln_fp16_top_of_range(dvt, device):
    """fp16 x and dy between 3e4 and 6e4 in magnitude: sums and squares far beyond fp16 in fp32 arithmetic; y and dx are of
    ordinary size again"""
    for d in (40, 2056):
        g = LR.gen(12000 + d)
        gamma, beta = LR.ln_params(d, g)
        x = LR.fp16_top_rows(5, d, g)
        dy = LR.fp16_top_rows(5, d, g)
        _fwd_dense(dvt.ops, device, x, gamma, beta, torch.float16, f"fp16 top d={d}")
        _bwd_dense(dvt.ops, device, dy, x, gamma, beta, torch.float16, None, f"fp16 top d={d}")


# ---------------------------------------------------------------- cross-entropy on integer labels
CE_M = [1, 15, 16, 17, 33]                    # sixteen waves, wave w takes rows w, w + 16, ...
CE_C = [1, 63, 64, 65, 305]                   # lanes stride by 64
IGNORE = -100


def _ce_run(ops, device, logits, labels, tag, ld=None, ignore_index=IGNORE):
    """forward and backward through ops on logits [M, C] (at a leading dimension ``ld`` > C: inside a NaN-padded buffer);
    -> (loss, lse, dlogits) on the CPU, with lse[0:M], lse[M] and, where the loss is a number, the loss judged"""
    M, Cc = logits.shape
    if ld is None:
        dev = logits.to(device)
    else:
        buf, chk = poisoned((M, ld), logits.dtype, device)
        buf[:, :Cc] = logits.to(device)
        dev = buf[:, :Cc]
    lab = labels.to(device)
    with guarded(ops):
        loss, lse = ops.ce_labels_fwd(dev, lab, ignore_index)
    loss, lse = loss.cpu(), lse.cpu()
    rl, rlse, rcount = LR.ce_labels(logits.double(), labels, ignore_index)
    cl, clse, ccount = LR.ce_labels(logits.float(), labels, ignore_index)
    R.assert_close(lse[:M], rlse, clse, logits.double().abs().max(1).values, f"lse {tag}")
    R.assert_close(lse[M:], rcount.reshape(1), ccount.reshape(1), 0.0, f"count {tag}")
    assert float(lse[M]) == float(rcount)
    if math.isnan(float(rl)):
        assert math.isnan(float(loss)), f"loss {tag}: {float(loss)} where the reference is NaN"
    else:
        R.assert_close(loss, rl.reshape(1), cl.reshape(1), float(logits.double().abs().max()), f"loss {tag}")
    # backward from the contract's own forward outputs (the CPU fp32 chain's lse, the count)
    gloss = torch.tensor([1.7])
    handed = torch.cat([clse, ccount.reshape(1)])
    with guarded(ops):
        dl = ops.ce_labels_bwd(dev, lab, handed.to(device), gloss.to(device), ignore_index)
    if ld is not None:
        chk()
    return loss, lse, dl.cpu(), (clse, ccount, gloss)


def _ce_judge_bwd(dl, logits, labels, handed, tag, rows=None, ignore_index=IGNORE):
    clse, ccount, gloss = handed
    ref = LR.ce_labels_bwd(logits.double(), labels, clse.double(), ccount.double(), gloss.double(), ignore_index)
    chain = LR.ce_labels_bwd(logits.float(), labels, clse, ccount, gloss, ignore_index)
    sel = slice(None) if rows is None else rows
    R.assert_close(dl[sel], ref[sel], chain[sel], float(gloss) / max(float(ccount), 1.0), f"dlogits {tag}")
    ignored = labels == ignore_index
    assert bool((dl[ignored].float() == 0).all()), f"dlogits {tag}: an ignored row's gradient is not exactly zero"


@pytest.mark.parametrize("name", DT)
def test_ce_labels(dvt, device, name):
    """every M x C; all the rows of wave 1 (rows 1, 17, 33) and row 2 are ignored"""
    dtype = R.DTYPES[name]
    for M in CE_M:
        for Cc in CE_C:
            logits, labels = LR.ce_case(M, Cc, dtype, LR.gen(M * 1000 + Cc))
            tag = f"{name} M={M} C={Cc}"
            _, _, dl, handed = _ce_run(dvt.ops, device, logits, labels, tag)
            _ce_judge_bwd(dl, logits, labels, handed, tag)


@pytest.mark.parametrize("name", DT)
def test_ce_labels_padded_rows(dvt, device, name):
    """logits at a leading dimension above C, NaN between the rows: nothing of the padding may reach an output"""
    dtype = R.DTYPES[name]
    for M, Cc, ld in ((17, 65, 72), (33, 1, 8), (16, 305, 311)):
        logits, labels = LR.ce_case(M, Cc, dtype, LR.gen(M * 1000 + Cc + 1))
        tag = f"{name} M={M} C={Cc} ld={ld}"
        _, _, dl, handed = _ce_run(dvt.ops, device, logits, labels, tag, ld=ld)
        _ce_judge_bwd(dl, logits, labels, handed, tag)


@pytest.mark.parametrize("name", DT)
def test_ce_labels_all_ignored(dvt, device, name):
    """no counted row: the loss is NaN (torch's mean over no rows), the count 0, and every gradient exactly zero although
    gloss / count is infinite"""
    logits, labels = LR.ce_case(17, 65, R.DTYPES[name], LR.gen(77), ignored="all")
    loss, lse, dl, _ = _ce_run(dvt.ops, device, logits, labels, f"{name} all ignored")
    assert math.isnan(float(loss)) and float(lse[17]) == 0.0
    assert bool((dl.float() == 0).all())


@pytest.mark.parametrize("name", DT)
def test_ce_labels_out_of_range_label(dvt, device, name):
    """one label >= C (not ignore_index): the loss is NaN and that row's gradient is NaN, every other row is as without
    it (the row is counted), the ignored rows stay exactly zero, and nothing outside the outputs is touched"""
    M, Cc, bad = 17, 65, 5
    logits, labels = LR.ce_case(M, Cc, R.DTYPES[name], LR.gen(78))
    labels[bad] = Cc
    tag = f"{name} label {Cc} of {Cc} classes"
    loss, lse, dl, handed = _ce_run(dvt.ops, device, logits, labels, tag)
    assert math.isnan(float(loss)) and float(lse[M]) == float((labels != IGNORE).sum())
    assert bool(torch.isnan(dl[bad].float()).all())
    _ce_judge_bwd(dl, logits, labels, handed, tag, rows=[r for r in range(M) if r != bad])
