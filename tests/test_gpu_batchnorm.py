"""Every BatchNorm and max-pool kernel of csrc/conv.hip called directly through ops.*, each output judged elementwise
against the float64 statement of tests/batchnorm_ref.py under the rule of tests/rowwise_ref.py (4 x the fp32 chain's own
error plus one fp32 ulp; a 16-bit output is the float64 result rounded to the dtype or a neighbouring value), and exactly
where the inputs make the kernels' sums exact (integer-valued maps, synthetic partial rows, dyadic stem maps), at the
smallest shapes that reach each path.

Operands are rounded to the kernel's dtype before the reference and the kernel see them; the forward and the backward are
handed the float64 reference's mean / invstd rounded to fp32, so each is judged on its own.  Outputs ops allocates sit in
the NaN bands of ``guarded``; destinations the caller owns come from ``poisoned`` (tests/guards.py).
tests/test_batchnorm_coverage.py ties every kernel symbol of the built library to a parameter set of this file.

What each shape is there for (B = tests/batchnorm_ref.py, whose mirrors say which kernel, CL and loop tier a shape reaches):
  WIDTHS      8, 16, 64: vc = C / 8 column vectors (1, 2, 8) and 256, 128, 32 row lanes; 144 and 264: the divisor search
              (vc = 18 leaves 4 threads idle, vc = 11 three); 296: 37 column vectors have no divisor, the power-of-two form
              with a ragged second block column; 512: vc = 32, two block columns.  C <= 256 finalizes with CL = 8 column
              lanes (PL = 128 part lanes), 264 / 296 / 512 with CL = 32 (PL = 32).
  row_counts  1, 3, 4, 5 rows, and one less / one more than one trip of a workgroup's row lanes (4 rows in flight per lane).
  SHORT_LAST  C = 64, 5003 rows: 39 workgroups of 129 rows = four rows per lane and a fifth for lane 0, the last one 101.
  grid cap    C = 8, rows = 4 * lanes + 3: the row-streaming kernels' grid is capped at 8 workgroups per compute unit, every
              lane makes one full trip of four rows and three lanes a second one (the forward and the backward each have
              their test and share the maps).
  PARTS       partial-row counts around PL and the loop tiers of bn_finalize_kernel (4 rows per trip from 3 PL + 1 parts, 8
              from 7 PL + 1) as far as parts <= 256 allows, and around the fold (257, 300: some of the 64 fold blocks are
              empty; 6143 / 6145: per_block = 96 / 97, either side of the fold's four-way loop; 8200).
  BIG         C = 8 at 2^20 rows: 1024 parts, the 8-row tier of bn_finalize_kernel<0, 8>; C = 512 at 16384 rows: 512 parts,
              the 16-row tier of <0, 32>.  The 16-row tier of <., 8> needs more than 15 * 128 = 1920 partial rows: bn_parts
              stops at 1024 and the fold hands over 64, so no caller can supply them and no case is contorted for it."""
import ctypes as C_
import functools
import math

import pytest
import torch

from tests import batchnorm_ref as B
from tests import rowwise_ref as R
from tests.guards import guarded, poisoned

pytestmark = pytest.mark.gpu

DT = ["fp32", "bf16", "fp16"]
WIDTHS = [8, 16, 64, 144, 264, 296, 512]
SHORT_LAST = (5003, 64)
SCALAR_WIDTHS = [1, 5, 45, 257]
MISALIGNED_C = 16
# (k, stride, pad): the stem's pool (its own backward kernel), three generic ones, and one whose tap indices pass 8
POOLS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2)]
POOL_MAPS = [(9, 11), (12, 16), (1, 5), (7, 2)]          # odd / even H and W, H = 1, W = 2
STEM_MAPS = [(2, 2), (2, 6), (9, 11), (12, 16), (16, 12)]
STEM_WIDTHS = [16, 64]
PARTS = {8: [1, 127, 128, 129, 256], 264: [1, 31, 32, 33, 96, 97, 127, 128, 129, 224, 225, 255, 256]}
FOLD_PARTS = [257, 300, 6143, 6145, 8200]
BIG = [(1 << 20, 8), (16384, 512)]


def row_counts(C):
    trip = B.ROW_UNROLL * B.row_lanes(C)
    return [1, 3, 4, 5, trip - 1, trip + 1]


def _hw_id(hw):
    return f"{hw[0]}x{hw[1]}"


def _pool_id(p):
    return f"k{p[0]}s{p[1]}p{p[2]}"


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


def _d(device, *ts):
    out = [None if t is None else t.to(device) for t in ts]
    return out if len(out) > 1 else out[0]


def _off_by_one(t, device):
    """t on the device, one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


# ---------------------------------------------------------------- statistics
def _stats(ops, device, x, tag, exact=False):
    with guarded(ops):
        mean, invstd = ops.bn_stats(_d(device, x), None, None, B.EPS, 0.1)
    if exact:
        x64 = x.double()
        B.check_exact_stats(mean.cpu(), invstd.cpu(), x64.mean(0), x64.var(0, unbiased=False), tag)
    else:
        B.check_stats(mean.cpu(), invstd.cpu(), x, tag)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_bn_stats(dvt, device, name, C):
    """ordinary maps under the rule; integer maps (columns of mean 100 and spread +-3 among them) exactly"""
    dtype = R.DTYPES[name]
    for rows in row_counts(C) + ([SHORT_LAST[0]] if C == SHORT_LAST[1] else []):
        g = B.gen(1000 + 7 * C + rows)
        _stats(dvt.ops, device, B.feature_map(rows, C, dtype, g), f"{name} rows={rows} C={C}")
        _stats(dvt.ops, device, B.integer_map(rows, C, dtype, g), f"{name} integer rows={rows} C={C}", exact=True)


@pytest.mark.parametrize("shape", BIG, ids=[f"{r}x{c}" for r, c in BIG])
@pytest.mark.parametrize("name", DT)
def test_bn_stats_big_integer_maps(dvt, device, name, shape):
    """the finalize tiers only real maps reach (see BIG above), on integer data: every sum is exact"""
    rows, C = shape
    parts, _ = B.bn_parts(rows, C)
    assert (parts, B.finalize_tiers(parts, B.finalize_cl(C))[0]) == {8: (1024, 8), 512: (512, 16)}[C]
    _stats(dvt.ops, device, B.integer_map(rows, C, R.DTYPES[name], B.gen(rows + C)), f"{name} integer rows={rows} C={C}", exact=True)


@pytest.mark.parametrize("C", [16, 264])
@pytest.mark.parametrize("name", DT)
def test_bn_running_stats(dvt, device, name, C):
    """momentum 0.1 and 1.0 from non-trivial starting values, rows = 1 (no unbias factor) and 37, c_valid in {C, C - 3,
    C - 8}: the running arrays have C elements here, and those beyond c_valid must keep what they held"""
    dtype, ops = R.DTYPES[name], dvt.ops
    for rows in (1, 37):
        for momentum in (0.1, 1.0):
            for c_valid in (C, C - 3, C - 8):
                g = B.gen(2000 + C + rows)
                x = B.feature_map(rows, C, dtype, g)
                rm0 = torch.randn(C, generator=g) * 2.0 + 1.0
                rv0 = torch.rand(C, generator=g) * 3.0 + 0.5
                rm, chk_m = poisoned((C,), torch.float32, device)
                rv, chk_v = poisoned((C,), torch.float32, device)
                rm.copy_(_d(device, rm0)); rv.copy_(_d(device, rv0))
                with guarded(ops):
                    mean, invstd = ops.bn_stats(_d(device, x), rm, rv, B.EPS, momentum, c_valid=c_valid)
                chk_m(); chk_v()
                tag = f"{name} rows={rows} C={C} momentum={momentum} c_valid={c_valid}"
                B.check_stats(mean.cpu(), invstd.cpu(), x, tag)
                B.check_running(rm.cpu(), rv.cpu(), x, rm0, rv0, momentum, c_valid, tag)


def _from_partials(ops, device, C, parts, tag):
    partial, rows, mean64, var64 = B.integer_partials(parts, C, B.gen(3000 + C + parts))
    buf, chk = poisoned(tuple(partial.shape), torch.float32, device)
    buf.copy_(_d(device, partial))
    rm0, rv0 = torch.full((C,), 2.0), torch.full((C,), 3.0)
    rm, chk_m = poisoned((C,), torch.float32, device)
    rv, chk_v = poisoned((C,), torch.float32, device)
    rm.copy_(_d(device, rm0)); rv.copy_(_d(device, rv0))
    with guarded(ops):
        mean, invstd = ops.bn_stats_from_partials(buf, parts, rows, C, rm, rv, B.EPS, 0.5, c_valid=C - 3)
    chk(); chk_m(); chk_v()
    B.check_exact_stats(mean.cpu(), invstd.cpu(), mean64, var64, tag)
    assert torch.equal(buf[:parts].cpu(), partial[:parts]), f"{tag}: the partial rows were changed"
    if parts <= B.FOLD_ABOVE:
        assert bool(torch.isnan(buf[parts:]).all()), f"{tag}: the tail was written without a fold"
    # the running statistics from exact batch statistics: 0.5 old + 0.5 new, the variance unbiased
    ref = B.running_update(rm0.double(), rv0.double(), mean64, var64, rows, 0.5, C - 3)
    chain = B.running_update(rm0, rv0, mean64.float(), var64.float(), rows, 0.5, C - 3)
    assert torch.equal(rm.cpu()[C - 3:], rm0[C - 3:]) and torch.equal(rv.cpu()[C - 3:], rv0[C - 3:]), f"{tag}: beyond c_valid"
    R.assert_close(rm.cpu(), ref[0], chain[0], torch.maximum(mean64.abs(), rm0.double()), f"running_mean {tag}")
    R.assert_close(rv.cpu(), ref[1], chain[1], torch.maximum(var64.abs(), rv0.double()), f"running_var {tag}")


PARTIALS = [(C, parts) for C in (8, 264) for parts in PARTS[C] + FOLD_PARTS]


@pytest.mark.parametrize("C,parts", PARTIALS, ids=[f"{c}-{p}" for c, p in PARTIALS])
def test_bn_stats_from_partials(dvt, device, C, parts):
    """synthetic integer partial rows (fp32 whatever the map's dtype, so there is one case per shape): the expected mean
    and variance are exact.  The buffer has parts + 64 rows, as the fold requires; its tail starts as NaN."""
    _from_partials(dvt.ops, device, C, parts, f"C={C} parts={parts}")


@pytest.mark.parametrize("C", [1, 255, 257])
def test_bn_eval_invstd(dvt, device, C):
    g = B.gen(3500 + C)
    var = torch.rand(C, generator=g) * 4.0
    var[0] = 0.0
    with guarded(dvt.ops):
        out = dvt.ops.bn_eval_invstd(_d(device, var), B.EPS)
    R.assert_close(out.cpu(), R.ref64(B.rsqrt_eps, var, eps=B.EPS), R.fp32_chain(B.rsqrt_eps, var, eps=B.EPS), 0.0, f"invstd C={C}")


# ---------------------------------------------------------------- forward
@functools.lru_cache(maxsize=3)                   # (a grid-cap map is built once for its forward and its backward test)
def _fwd_case(rows, C, dtype, seed, c_valid=None):
    """-> (x, residual, gamma, beta, mean, invstd), shared between callers: none of them writes into it"""
    g = B.gen(seed)
    x = B.feature_map(rows, C, dtype, g)
    res = B.randn((rows, C), dtype, g)
    gamma, beta = B.bn_params(C if c_valid is None else c_valid, g, both_signs=True)
    mean, invstd = B.stats32(x)
    if rows == 1:                                               # (a single row normalises to beta: keep y a function of x)
        mean, invstd = mean - 0.5, torch.full_like(invstd, 1.25)
    return x, res, gamma, beta, mean, invstd


def _fwd(ops, device, x, res, gamma, beta, mean, invstd, relu, want_mask, tag, c_valid=0):
    with guarded(ops):
        out = ops.bn_apply_fwd(*_d(device, x, mean, invstd, gamma, beta, res), relu, want_mask=want_mask, c_valid=c_valid)
    y, mask = out if want_mask else (out, None)
    assert y.dtype == x.dtype and y.shape == x.shape
    B.check_fwd(y.cpu(), None if mask is None else mask.cpu(), x, mean, invstd, gamma, beta, res, relu, tag)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("name", DT)
def test_bn_apply_fwd(dvt, device, name, res, mask):
    """bn_apply_fwd_kernel<T, RES, MASK> at every width and row count, with and without the ReLU; the mask bytes are judged
    against the y the kernel stored"""
    dtype = R.DTYPES[name]
    for C in WIDTHS:
        for rows in row_counts(C) + ([SHORT_LAST[0]] if C == SHORT_LAST[1] else []):
            x, r, gamma, beta, mean, invstd = _fwd_case(rows, C, dtype, 4000 + 7 * C + rows)
            for relu in (True, False):
                _fwd(dvt.ops, device, x, r if res else None, gamma, beta, mean, invstd, relu, mask,
                     f"{name} res={res} mask={mask} relu={relu} rows={rows} C={C}")


@pytest.mark.parametrize("C", [16, 264])
@pytest.mark.parametrize("name", DT)
def test_bn_apply_fwd_c_valid(dvt, device, name, C):
    """gamma / beta have c_valid elements: C - 3 leaves the last group ragged, C - 8 drops it whole; the padded channels are
    gamma = beta = 0 (with a residual they are the residual)"""
    dtype = R.DTYPES[name]
    for c_valid in (C - 3, C - 8):
        x, r, gamma, beta, mean, invstd = _fwd_case(37, C, dtype, 4500 + C, c_valid=c_valid)
        gb, chk_g = poisoned((c_valid,), torch.float32, device)        # (nothing beyond c_valid may be read: it is NaN)
        bb, chk_b = poisoned((c_valid,), torch.float32, device)
        gb.copy_(_d(device, gamma)); bb.copy_(_d(device, beta))
        for res, mask in ((False, True), (True, False)):
            with guarded(dvt.ops):
                out = dvt.ops.bn_apply_fwd(*_d(device, x, mean, invstd), gb, bb, _d(device, r) if res else None, True,
                                           want_mask=mask, c_valid=c_valid)
            y, mb = out if mask else (out, None)
            chk_g(); chk_b()
            B.check_fwd(y.cpu(), None if mb is None else mb.cpu(), x, mean, invstd, gamma, beta, r if res else None, True,
                        f"{name} C={C} c_valid={c_valid} res={res}")
            if not res:
                assert bool((y[:, c_valid:] == 0).all())


# ---------------------------------------------------------------- backward
def _bwd_case(rows, C, dtype, seed, src, relu, c_valid=None):
    """-> (dy, z, y, mask, on, gamma, beta, mean, invstd): ``src`` names where the ReLU mask comes from -- "mask" bytes, the
    stored "y", or "z" (recomputed from beta; z is then cleared of the margin around the zero of the pre-activation).  The
    y handed over is the float64 forward rounded to the dtype, so the reference decides from the same y."""
    x, res, gamma, beta, mean, invstd = _fwd_case(rows, C, dtype, seed, c_valid)
    dy = B.randn((rows, C), dtype, B.gen(seed + 1))
    y = mask = on = None
    if relu and src == "z":
        gp, bp = B.padded(gamma, C), B.padded(beta, C)
        x = B.clear_mask_margin(x, mean, invstd, gp, bp)
        on = (B.mask_margin(x, mean, invstd, gp, bp)[0] > 0).double()
    elif relu:
        y = R.ref64(B.bn_fwd, x, mean, invstd, gamma, beta, res, relu=True).to(dtype)
        on = (y.float() > 0).double()
        if src == "mask":
            mask, y = B.mask_bytes(y), None
    return dy, x, y, mask, on, gamma, beta, mean, invstd


def _bwd(ops, device, case, relu, training, dres, tag, *, c_valid=0, dg0=None, db0=None, report=False):
    dy, x, y, mask, on, gamma, beta, mean, invstd = case
    kw = {}
    chks = []
    if dg0 is not None:
        n = dg0.shape[0]
        kw["dgamma"], c1 = poisoned((n,), torch.float32, device)
        kw["dbeta"], c2 = poisoned((n,), torch.float32, device)
        kw["dgamma"].copy_(_d(device, dg0)); kw["dbeta"].copy_(_d(device, db0))
        kw["accumulate"] = True
        chks = [c1, c2]
    from_z = relu and y is None and mask is None
    with guarded(ops):
        dx, dr, dg, db = ops.bn_bwd(*_d(device, dy, x, y, mean, invstd, gamma), relu, training, dres,
                                    beta=_d(device, beta) if from_z else None, mask=_d(device, mask), c_valid=c_valid, **kw)
    for c in chks:
        c()
    assert (dr is not None) == dres and dg.shape[0] == (c_valid or x.shape[1])
    B.check_bwd(dx.cpu(), dr.cpu() if dres else None, dg.cpu(), db.cpu(), dy, x, on, mean, invstd, gamma, training, tag,
                dg0=dg0, db0=db0, c_valid=c_valid or None, report=report)


BWD_SRC = [("z", False), ("z", True), ("y", False), ("y", True), ("mask", False), ("mask", True)]


@pytest.mark.parametrize("src,dres", BWD_SRC, ids=[f"{s}-{'dres' if d else 'nodres'}" for s, d in BWD_SRC])
@pytest.mark.parametrize("name", DT)
def test_bn_bwd(dvt, device, name, src, dres):
    """every (mask source, dres) pair, train and eval, at every width; the ReLU is on except for (z, dres), which a ReLU
    layer cannot ask for (a residual branch needs the mask bytes or y): that pair and relu=False run MSRC 0 without a ReLU"""
    dtype = R.DTYPES[name]
    for C in WIDTHS:
        for rows in (1, 5, row_counts(C)[-1]) + ((SHORT_LAST[0],) if C == SHORT_LAST[1] else ()):
            for relu in ((False,) if (src, dres) == ("z", True) else (True, False) if src == "z" else (True,)):
                case = _bwd_case(rows, C, dtype, 5000 + 7 * C + rows, src, relu)
                for training in (True, False):
                    _bwd(dvt.ops, device, case, relu, training, dres,
                         f"{name} src={src} dres={dres} relu={relu} train={training} rows={rows} C={C}")


@pytest.mark.parametrize("C", [16, 264])
@pytest.mark.parametrize("name", DT)
def test_bn_bwd_accumulate_and_c_valid(dvt, device, name, C):
    """accumulate onto non-zero dgamma / dbeta; c_valid < C: gamma, beta, dgamma and dbeta have c_valid elements, the
    padded channels' dx and dres are exact zeros under a recomputed mask"""
    dtype = R.DTYPES[name]
    for c_valid in (0, C - 3, C - 8):
        n = c_valid or C
        for src in ("z", "y", "mask"):
            g = B.gen(5500 + C + n)
            case = _bwd_case(37, C, dtype, 5600 + C + n, src, True, c_valid=c_valid or None)
            dg0, db0 = 3.0 * torch.randn(n, generator=g), 3.0 * torch.randn(n, generator=g)
            tag = f"{name} src={src} C={C} c_valid={c_valid}"
            _bwd(dvt.ops, device, case, True, True, src != "z", f"{tag} accumulate", c_valid=c_valid, dg0=dg0, db0=db0)
            _bwd(dvt.ops, device, case, True, False, False, f"{tag} overwrite", c_valid=c_valid)


@pytest.mark.parametrize("name", DT)
def test_bn_integer_gradients_sum_exactly(dvt, device, name):
    """dbeta from integer dy is exact (every partial below 2^24, double across the partial rows), at the short-last-block
    shape and at a width of each CL"""
    dtype = R.DTYPES[name]
    for rows, C in (SHORT_LAST, (37, 264), (4099, 16)):
        g = B.gen(5800 + C)
        x = B.feature_map(rows, C, dtype, g)
        dy = B.integer_grad(rows, C, dtype, g)
        mean, invstd = B.stats32(x)
        gamma, _ = B.bn_params(C, g)
        with guarded(dvt.ops):
            _, _, _, db = dvt.ops.bn_bwd(*_d(device, dy, x, None, mean, invstd, gamma), False, True, False)
        assert torch.equal(db.cpu().double(), dy.double().sum(0)), f"{name} rows={rows} C={C}: dbeta of integer dy is not exact"


# ---------------------------------------------------------------- the grid cap of the row-streaming kernels
def _cap_rows(dvt):
    """C = 8 is one column vector, so every thread of the capped grid (8 workgroups of 256 per compute unit) is a row lane;
    rows = 4 * lanes + 3 is one full trip of every lane and three rows of a second"""
    return B.ROW_UNROLL * 8 * 256 * _cu_count(dvt) + 3


@pytest.mark.parametrize("name", DT)
def test_bn_apply_fwd_grid_cap(dvt, device, name):
    """the forward at the grid cap, with residual and mask bytes (about 2 M rows of 8 channels: the largest map here)"""
    rows = _cap_rows(dvt)
    x, res, gamma, beta, mean, invstd = _fwd_case(rows, 8, R.DTYPES[name], 6000)
    _fwd(dvt.ops, device, x, res, gamma, beta, mean, invstd, True, True, f"{name} grid cap rows={rows} C=8")


@pytest.mark.parametrize("name", DT)
def test_bn_bwd_grid_cap(dvt, device, name):
    """the backward at the grid cap, from mask bytes, with dres: the largest row count dgamma and dbeta are summed over in
    this file; their worst error against the budget is printed"""
    rows = _cap_rows(dvt)
    case = _bwd_case(rows, 8, R.DTYPES[name], 6000, "mask", True)
    _bwd(dvt.ops, device, case, True, True, True, f"{name} grid cap rows={rows} C=8", report=True)


# ---------------------------------------------------------------- the scalar kernels
def _scalar_calls(ops, device, name, rows, C, move, tag):
    """bn_stats, bn_apply_fwd, bn_bwd (with y, and with the mask recomputed from beta) on the scalar path; ``move`` puts an
    operand on the device (where C % 8 == 0, off its 16-byte boundary)"""
    dtype = R.DTYPES[name]
    x, res, gamma, beta, mean, invstd = _fwd_case(rows, C, dtype, 7000 + C + rows)
    with guarded(ops):
        m, s = ops.bn_stats(move(x), None, None, B.EPS, 0.1)
    B.check_stats(m.cpu(), s.cpu(), x, tag)
    xi = B.integer_map(rows, C, dtype, B.gen(7100 + C))
    with guarded(ops):
        m, s = ops.bn_stats(move(xi), None, None, B.EPS, 0.1)
    B.check_exact_stats(m.cpu(), s.cpu(), xi.double().mean(0), xi.double().var(0, unbiased=False), f"{tag} integer")
    for r, relu in ((None, True), (res, True), (res, False)):
        with guarded(ops):
            y = ops.bn_apply_fwd(move(x), *_d(device, mean, invstd, gamma, beta, r), relu)
        B.check_fwd(y.cpu(), None, x, mean, invstd, gamma, beta, r, relu, f"{tag} res={r is not None} relu={relu}")
    for src, relu, dres in (("y", True, True), ("y", True, False), ("z", True, False), ("z", False, True)):
        dy, xc, y, _, on, *_ = case = _bwd_case(rows, C, dtype, 7000 + C + rows, src, relu)
        for training in (True, False):
            with guarded(ops):
                dx, dr, dg, db = ops.bn_bwd(move(dy), *_d(device, xc, y, mean, invstd, gamma), relu, training, dres,
                                            beta=_d(device, beta) if (relu and src == "z") else None)
            B.check_bwd(dx.cpu(), dr.cpu() if dres else None, dg.cpu(), db.cpu(), dy, xc, on, mean, invstd, gamma, training,
                        f"{tag} src={src} relu={relu} train={training}")


@pytest.mark.parametrize("C", SCALAR_WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_bn_scalar(dvt, device, name, C):
    """C % 8 != 0: one thread per column (statistics) or per element (apply); 300 rows make more than one partial row"""
    for rows in (1, 5, 300):
        assert rows < 300 or B.bn_parts(rows, C)[0] > 1
        _scalar_calls(dvt.ops, device, name, rows, C, lambda t: _d(device, t), f"{name} scalar rows={rows} C={C}")


@pytest.mark.parametrize("name", DT)
def test_bn_scalar_misaligned(dvt, device, name):
    """C = 16 with the map (x for the statistics and the forward, dy for the backward) one element past a 16-byte boundary"""
    for rows in (5, 300):
        _scalar_calls(dvt.ops, device, name, rows, MISALIGNED_C, lambda t: _off_by_one(t, device),
                      f"{name} misaligned rows={rows} C={MISALIGNED_C}")


def _refused(ops, call):
    """the call raises the wrapper's unsupported error and launches nothing: every output it allocated is still NaN"""
    with pytest.raises(RuntimeError, match="need C % 8 == 0 and 16-byte aligned buffers"):
        with guarded(ops) as g:
            call()
    torch.cuda.synchronize()
    assert g.live and all(bool(torch.isnan(buf).all()) for buf, _ in g.live), "a refused call wrote an output"


@pytest.mark.parametrize("name", DT)
def test_bn_scalar_path_refuses_mask_and_channel_padding(dvt, device, name):
    ops, dtype = dvt.ops, R.DTYPES[name]
    for C, move in ((45, lambda t: _d(device, t)), (MISALIGNED_C, lambda t: _off_by_one(t, device))):
        rows = 5
        dy, x, y, _, _, gamma, beta, mean, invstd = _bwd_case(rows, C, dtype, 7500 + C, "y", True)
        dev = _d(device, mean, invstd, gamma, beta)
        mask = torch.zeros((rows, max(C // 8, 1)), dtype=torch.uint8, device=device)[:, :C // 8].contiguous()
        _refused(ops, lambda: ops.bn_apply_fwd(move(x), *dev, None, True, want_mask=True))
        _refused(ops, lambda: ops.bn_apply_fwd(move(x), *dev, None, True, c_valid=C - 1))
        _refused(ops, lambda: ops.bn_bwd(move(dy), *_d(device, x, y, mean, invstd, gamma), True, True, False, c_valid=C - 1))
        if C % 8 == 0:
            _refused(ops, lambda: ops.bn_bwd(move(dy), *_d(device, x, None, mean, invstd, gamma), True, True, False, mask=mask))


# ---------------------------------------------------------------- max-pool
def _pool_inputs(rows, C, dtype, g):
    """ordinary values; many ties (a rectified map quantised to quarters); negative values only"""
    x = torch.randn(rows, C, generator=g, dtype=torch.float64)
    return {"random": x.to(dtype), "ties": ((x.clamp_min(0) * 4).round() / 4).to(dtype), "negative": (-0.5 - x.abs()).to(dtype)}


def _pool(ops, device, x, N, C, H, W, k, stride, pad, g, tag, move=None):
    move = move or (lambda t: _d(device, t))
    geom = dict(N=N, H=H, W=W, k=k, stride=stride, pad=pad)
    with guarded(ops):
        y, idx = ops.maxpool_fwd(move(x), N, C, H, W, k, stride, pad)
    ry, rtap = B.maxpool_fwd(x, **geom)
    B.check_maxpool_fwd(y.cpu(), idx.cpu().view(-1, C), x, geom, tag)
    for exact in (False, True):
        dy = B.integer_grad(*ry.shape, x.dtype, g) if exact else B.randn(tuple(ry.shape), x.dtype, g)
        with guarded(ops):
            dx = ops.maxpool_bwd(move(dy), idx, N, C, H, W, k, stride, pad)
        B.check_maxpool_bwd(dx.cpu(), dy, rtap, geom, tag, exact=exact)


@pytest.mark.parametrize("pool", POOLS, ids=[_pool_id(p) for p in POOLS])
@pytest.mark.parametrize("name", DT)
def test_maxpool(dvt, device, name, pool):
    """values and tap bytes exactly; the backward under the rule, and exactly for integer dy.  (3, 2, 1) runs
    maxpool_bwd_k3s2p1_kernel, the others maxpool_bwd_vec_kernel.  N = 3, C = 16: 6 Ho Wo items, no multiple of 256"""
    k, stride, pad = pool
    N, C, ran = 3, 16, 0
    for H, W in POOL_MAPS:
        if H + 2 * pad < k or W + 2 * pad < k:
            continue
        ran += 1
        g = B.gen(8000 + 100 * H + W + k)
        assert (N * math.prod(B.out_hw(H, W, k, stride, pad)) * (C // 8)) % 256
        for kind, x in _pool_inputs(N * H * W, C, R.DTYPES[name], g).items():
            _pool(dvt.ops, device, x, N, C, H, W, k, stride, pad, g, f"{name} {_pool_id(pool)} {H}x{W} {kind}")
    assert ran >= 2


@pytest.mark.parametrize("C", SCALAR_WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_maxpool_scalar(dvt, device, name, C):
    """C % 8 != 0: maxpool_fwd_kernel and maxpool_bwd_kernel, one thread per element"""
    N = 3
    for (k, stride, pad), (H, W) in (((3, 2, 1), (9, 11)), ((5, 2, 2), (7, 2)), ((2, 2, 0), (12, 16))):
        g = B.gen(8500 + C + k)
        for kind, x in _pool_inputs(N * H * W, C, R.DTYPES[name], g).items():
            _pool(dvt.ops, device, x, N, C, H, W, k, stride, pad, g, f"{name} scalar C={C} k{k}s{stride}p{pad} {H}x{W} {kind}")


@pytest.mark.parametrize("name", DT)
def test_maxpool_scalar_misaligned(dvt, device, name):
    N, C, H, W = 3, MISALIGNED_C, 9, 11
    g = B.gen(8600)
    for kind, x in _pool_inputs(N * H * W, C, R.DTYPES[name], g).items():
        _pool(dvt.ops, device, x, N, C, H, W, 3, 2, 1, g, f"{name} misaligned {kind}", move=lambda t: _off_by_one(t, device))


# ---------------------------------------------------------------- the fused stem
@pytest.mark.parametrize("hw", STEM_MAPS, ids=[_hw_id(hw) for hw in STEM_MAPS])
@pytest.mark.parametrize("C", STEM_WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_stem_fwd(dvt, device, name, C, hw):
    """BatchNorm (+ ReLU) + max-pool(3, 2, 1) in one pass against the reference chain -- the forward rounded to the dtype,
    then the pool -- pooled values and taps exactly, on dyadic maps (the pre-activation is exact in either order of
    evaluation; gamma of both signs) and on maps of zeros and ones.  relu=False in 16 bits is the compare form of the
    kernel, relu=True the packed-key form."""
    dtype, ops, N, (H, W) = R.DTYPES[name], dvt.ops, 3, hw
    g = B.gen(9000 + C + 100 * H + W)
    one, zero = torch.ones(C), torch.zeros(C)
    for kind, z, params in (("dyadic", B.stem_map(N * H * W, C, dtype, g), B.stem_params(C, g)),
                            ("ties", B.tie_map(N * H * W, C, dtype, g), (zero, one, one, zero))):
        for relu in (True, False):
            with guarded(ops):
                p, idx = ops.bn_relu_maxpool_fwd(*_d(device, z, *params), N, C, H, W, relu)
            B.check_stem_fwd(p.cpu(), idx.cpu().view(-1, C), z, *params, N, H, W, relu, f"{name} {kind} relu={relu} C={C} {H}x{W}")


@pytest.mark.parametrize("hw", STEM_MAPS, ids=[_hw_id(hw) for hw in STEM_MAPS])
@pytest.mark.parametrize("C", STEM_WIDTHS)
@pytest.mark.parametrize("name", DT)
def test_stem_bwd(dvt, device, name, C, hw):
    """bn_bwd_pooled: dy gathered from the pooled gradient by the tap bytes, the mask recomputed from z (dyadic: no bit in
    doubt).  Even H and W run the quad kernels, odd ones bn_colstats_kernel<T, 1, true> and bn_apply_bwd_pool_kernel."""
    dtype, ops, N, (H, W) = R.DTYPES[name], dvt.ops, 3, hw
    g = B.gen(9500 + C + 100 * H + W)
    z = B.stem_map(N * H * W, C, dtype, g)
    mean, invstd, gamma, beta = B.stem_params(C, g)
    assert B.inside_mask_margin(z, mean, invstd, gamma, beta) == 0
    on = (B.mask_margin(z, mean, invstd, gamma, beta)[0] > 0).double()
    for relu in (True, False):
        _, tap = B.stem_fwd(z, mean, invstd, gamma, beta, N, H, W, relu, dtype)
        dyp = B.randn(tuple(tap.shape), dtype, g)
        for training in (True, False):
            for acc in (False, True):
                dg0, db0 = 3.0 * torch.randn(C, generator=g), 3.0 * torch.randn(C, generator=g)
                dg, chk_g = poisoned((C,), torch.float32, device)
                db, chk_b = poisoned((C,), torch.float32, device)
                if acc:
                    dg.copy_(_d(device, dg0)); db.copy_(_d(device, db0))
                with guarded(ops):                                                 # (dx is ops' own)
                    dx, _, _ = ops.bn_bwd_pooled(*_d(device, dyp, tap.reshape(-1), z, mean, invstd, gamma, beta), N, H, W, relu,
                                                 training, dgamma=dg, dbeta=db, accumulate=acc)
                chk_g(); chk_b()
                tag = f"{name} relu={relu} train={training} acc={acc} C={C} {H}x{W}"
                dyfull = B.maxpool_bwd(dyp.double(), tap, N, H, W, 3, 2, 1)
                ops_ = (dyp, z, on if relu else None, mean, invstd, gamma)
                ref = R.ref64(B.stem_bwd, *ops_, tap=tap, N=N, H=H, W=W, training=training)
                chain = R.fp32_chain(B.stem_bwd, *ops_, tap=tap, N=N, H=H, W=W, training=training)
                m_dx, m_dg, m_db = B.bwd_mags(dyfull, z, on if relu else None, mean, invstd, gamma, training,
                                              dy_mag=B.maxpool_bwd(dyp.double().abs(), tap, N, H, W, 3, 2, 1))
                R.assert_close(dx.cpu(), ref[0], chain[0], m_dx, f"dx {tag}")
                for got, r, c, m, base, what in ((dg, ref[2], chain[2], m_dg, dg0, "dgamma"), (db, ref[3], chain[3], m_db, db0, "dbeta")):
                    if acc:
                        r, c, m = r + base.double(), c + base, torch.maximum(m, base.double().abs())
                    R.assert_close(got.cpu(), r, c, m, f"{what} {tag}")


# ---------------------------------------------------------------- for tests/test_batchnorm_cpu.py
def mask_recompute_cases():
    """(tag, z, mean, invstd, gamma, beta) of every call of this file whose ReLU mask is recomputed from z, as the tests
    above build them (gamma / beta zero-extended to C)"""
    for name in DT:
        dtype = R.DTYPES[name]
        for C in WIDTHS:
            for rows in (1, 5, row_counts(C)[-1]) + ((SHORT_LAST[0],) if C == SHORT_LAST[1] else ()):
                _, z, _, _, _, gamma, beta, mean, invstd = _bwd_case(rows, C, dtype, 5000 + 7 * C + rows, "z", True)
                yield f"test_bn_bwd {name} rows={rows} C={C}", z, mean, invstd, gamma, beta
        for C in (16, 264):
            for c_valid in (0, C - 3, C - 8):
                n = c_valid or C
                _, z, _, _, _, gamma, beta, mean, invstd = _bwd_case(37, C, dtype, 5600 + C + n, "z", True, c_valid=c_valid or None)
                yield f"test_bn_bwd_accumulate_and_c_valid {name} C={C} c_valid={c_valid}", z, mean, invstd, B.padded(gamma, C), B.padded(beta, C)
        for C, row_set in [(c, (1, 5, 300)) for c in SCALAR_WIDTHS] + [(MISALIGNED_C, (5, 300))]:
            for rows in row_set:
                _, z, _, _, _, gamma, beta, mean, invstd = _bwd_case(rows, C, dtype, 7000 + C + rows, "z", True)
                yield f"scalar {name} rows={rows} C={C}", z, mean, invstd, gamma, beta
        for C in STEM_WIDTHS:
            for H, W in STEM_MAPS:
                g = B.gen(9500 + C + 100 * H + W)
                z = B.stem_map(3 * H * W, C, dtype, g)
                yield (f"test_stem_bwd {name} C={C} {H}x{W}", z, *B.stem_params(C, g))
