"""The row, gating, loss and data-movement kernels called directly through ops.*, each against the float64 statement of
tests/rowwise_ref.py under that file's tolerance rule (4 x the fp32 chain's own error plus one fp32 ulp; a 16-bit output
is the float64 result rounded to the dtype or a neighbouring value), at edge shapes rather than workload shapes.

Every output a wrapper allocates is, for the duration of the call, a view into a larger NaN-filled buffer (``guarded``
stands in for torch.empty / torch.empty_like inside ops): the bands before and after must still be NaN afterwards, and no
NaN may be left inside.  Destinations the caller owns get the same bands from ``poisoned`` (both of tests/guards.py)."""
import math

import pytest
import torch

from tests import rowwise_ref as R
from tests.guards import guarded, poisoned

pytestmark = pytest.mark.gpu

DT = ["fp32", "bf16", "fp16"]
ROWS = [1, 3, 4, 5, 9]                        # four rows per workgroup: a part block, a whole one, one more than whole
DS = [1, 7, 63, 64, 65, 200]                  # lanes stride by 64
NS = [1, 7, 8, 9, 255, 257, 2051]


@pytest.fixture(scope="module")
def dvt(device):
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).to(dtype)


def _big_n(device):
    """just above the grid-stride kernels' grid (8 workgroups of 256 per CU): the stride loop runs twice"""
    return torch.cuda.get_device_properties(device).multi_processor_count * 8 * 256 + 77


def _edge_matrix(D, dtype, eps, gen):
    return torch.cat([R.l2norm_edge_rows(D, dtype, eps, gen), _randn((3, D), dtype, gen)], 0)       # 9 rows


# ---------------------------------------------------------------- wave-per-row kernels
@pytest.mark.parametrize("eps", [1e-12, 1e-8])
@pytest.mark.parametrize("name", DT)
def test_l2norm_rows(dvt, device, name, eps):
    dtype, ops, g = R.DTYPES[name], dvt.ops, _gen(11)
    for D in DS:
        full = _edge_matrix(D, dtype, eps, g)
        for rows in ROWS:
            x = torch.roll(full, rows, 0)[:rows].contiguous()
            with guarded(ops):
                y, inv = ops.l2norm_rows_fwd(x.to(device), eps)
            tag = f"{name} eps={eps} rows={rows} D={D}"
            R.assert_close(y.cpu(), R.ref64(R.l2norm_rows, x, eps=eps), R.fp32_chain(R.l2norm_rows, x, eps=eps), 0.0,
                           f"l2norm y {tag}")                      # (y = x * inv: its own magnitude is the scale)
            R.assert_close(inv.cpu(), R.ref64(R.l2norm_inv, x, eps=eps), R.fp32_chain(R.l2norm_inv, x, eps=eps), 0.0,
                           f"l2norm inv {tag}")
            # backward on the contract's own forward outputs (CPU fp32 chain), against float64 autograd of F.normalize
            y_c = R.fp32_chain(R.l2norm_rows, x, eps=eps, out_dtype=dtype)
            inv_c = R.fp32_chain(R.l2norm_inv, x, eps=eps)
            dy = _randn((rows, D), dtype, g)
            with guarded(ops):
                dx = ops.l2norm_rows_bwd(dy.to(device), y_c.to(device), inv_c.to(device), eps)
            ref = R.ref64(R.l2norm_rows_bwd, x, dy, eps=eps)
            chain = R.l2norm_rows_bwd_from_y(y_c.float(), inv_c, dy.float(), eps)
            y64, dy64, inv64 = y_c.double(), dy.double(), inv_c.double().unsqueeze(1)
            # what goes into an element: inv * dy_i and inv * y_i * <y, dy>, the dot product at the magnitude of the
            # products it sums (sum_j |y_j dy_j|: what any order of summation can lose, however the terms cancel)
            mag = inv64 * torch.maximum(dy64.abs(), y64.abs() * (y64 * dy64).abs().sum(1, keepdim=True))
            R.assert_close(dx.cpu(), ref, chain, mag, f"l2norm dx {tag}")


@pytest.mark.parametrize("eps", [1e-12, 1e-8])
@pytest.mark.parametrize("name", DT)
def test_cosine_rows(dvt, device, name, eps):
    from dvt_amd import metrics
    dtype, ops, g = R.DTYPES[name], dvt.ops, _gen(12)

    def run(a, b, tag):
        with guarded(ops):
            out = ops.cosine_rows(a.to(device), b.to(device), eps)
        ref = R.ref64(R.cosine_rows, a, b, eps=eps)
        a64, b64 = a.double(), b.double()
        cond = (a64 * b64).abs().sum(1) / (a64.norm(dim=1).clamp_min(eps) * b64.norm(dim=1).clamp_min(eps))
        R.assert_close(out.cpu(), ref, R.fp32_chain(R.cosine_rows, a, b, eps=eps), cond, f"cosine {tag}")
        assert torch.equal(out.cpu(), metrics.CosineSimilarity(dim=1, eps=eps)(a.to(device), b.to(device)).cpu())
        return out.cpu()

    for D in DS:
        full = _edge_matrix(D, dtype, eps, g)
        other = (0.5 * torch.flip(full, [0]).double() + 0.25 * full.double()      # (row 4 meets itself: stays below fp16's 65504)
                 + 0.125 * torch.randn(full.shape, generator=g, dtype=torch.float64).clamp(-4, 4) * full.double().abs().max(1, keepdim=True).values)
        other = other.to(dtype)
        assert bool(torch.isfinite(other.float()).all())
        for rows in ROWS:
            run(torch.roll(full, rows, 0)[:rows].contiguous(), torch.roll(other, rows, 0)[:rows].contiguous(),
                f"{name} eps={eps} rows={rows} D={D}")
    if eps == 1e-8:
        a, b = R.cosine_small_norm_pair(dtype)               # (fp16 holds 3e-6 as a subnormal: 50 and 67 steps of 2^-24)
        got = float(run(a, b, f"{name} small-norm pair"))
        assert got > 0.9, got                                # torch's 0.96, not the 0.0024 of a clamped product


@pytest.mark.parametrize("T", [0.1, 0.5])
def test_contrastive_rows(dvt, device, T):
    ops, g = dvt.ops, _gen(13)
    for M in (2, 4, 6, 130, 258):
        sim = R.contrastive_sim(M, T, g)
        with guarded(ops):
            loss, lse = ops.contrastive_fwd(sim.to(device), T)
        rl, rlse, rrow = R.ref64(R.contrastive_rows, sim, temperature=T)
        cl, clse, _ = R.fp32_chain(R.contrastive_rows, sim, temperature=T)
        rowmag = (sim.double().abs() / T).max(1).values
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss))
        R.assert_close(lse.cpu(), rlse, clse, rowmag, f"row_lse M={M} T={T}")
        # (a row's loss is the difference of two logits of magnitude |sim / T|: that, not the difference, is the operand)
        R.assert_close(loss.cpu().reshape(1), rl.reshape(1), cl.reshape(1), float(rowmag.max()), f"loss M={M} T={T}")
        gloss = torch.tensor([1.3])
        with guarded(ops):
            dsim = ops.contrastive_bwd(sim.to(device), clse.to(device), T, gloss.to(device))
        R.assert_close(dsim.cpu(), R.ref64(R.contrastive_dsim, sim, gloss, temperature=T),
                       R.fp32_chain(R.contrastive_dsim, sim, gloss, temperature=T), 1.3 / M / T, f"dsim M={M} T={T}")


# ---------------------------------------------------------------- grid-stride elementwise kernels
def _pairs(n, dtype, seed):
    """a, b, dy of n elements: the special values of a meet other special values in b"""
    a = R.elementwise_values(n, dtype, _gen(seed))
    b = torch.roll(R.elementwise_values(n, dtype, _gen(seed + 1)), 3)
    dy = _randn((n,), dtype, _gen(seed + 2))
    return a, b, dy


@pytest.mark.parametrize("name", DT)
def test_gate(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in NS + [_big_n(device)]:
        a, b, dy = _pairs(n, dtype, n)
        with guarded(ops):
            y = ops.gate_fwd(a.to(device), b.to(device))
        m = torch.maximum(a.double().abs(), b.double().abs())
        R.assert_close(y.cpu(), R.ref64(R.gate, a, b), R.fp32_chain(R.gate, a, b), m, f"gate_fwd {name} n={n}")
        with guarded(ops):
            da, db = ops.gate_bwd(dy.to(device), a.to(device), b.to(device))
        rda, rdb = R.ref64(R.gate_bwd, a, b, dy)
        cda, cdb = R.fp32_chain(R.gate_bwd, a, b, dy)
        R.assert_close(da.cpu(), rda, cda, torch.maximum(m, dy.double().abs()), f"gate_bwd da {name} n={n}")
        R.assert_close(db.cpu(), rdb, cdb, torch.maximum(m, (dy.double() * a.double()).abs()), f"gate_bwd db {name} n={n}")


@pytest.mark.parametrize("kind", [R.ACT_GELU, R.ACT_RELU, R.ACT_SIGMOID], ids=["gelu", "relu", "sigmoid"])
@pytest.mark.parametrize("name", DT)
def test_act(dvt, device, name, kind):
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in NS + [_big_n(device)]:
        x, _, dy = _pairs(n, dtype, 100 + n)
        with guarded(ops):
            y = ops.act_fwd(x.to(device), kind)
        R.assert_close(y.cpu(), R.ref64(R.act, x, kind=kind), R.fp32_chain(R.act, x, kind=kind), x.double().abs(),
                       f"act_fwd {name} kind={kind} n={n}")
        with guarded(ops):
            dx = ops.act_bwd(dy.to(device), x.to(device), kind)
        R.assert_close(dx.cpu(), R.ref64(R.act_bwd, x, dy, kind=kind), R.fp32_chain(R.act_bwd, x, dy, kind=kind),
                       torch.maximum(x.double().abs(), dy.double().abs()), f"act_bwd {name} kind={kind} n={n}")


@pytest.mark.parametrize("name", DT)
def test_axpby_f32(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in NS + [_big_n(device)]:
        src, _, _ = _pairs(n, dtype, 200 + n)
        dst, check = poisoned((n,), torch.float32, device)                  # NaN everywhere: beta = 0 must overwrite
        ops.axpby_f32_(dst, src.to(device), alpha=-1.5, beta=0.0)
        check()
        assert torch.equal(dst.cpu(), R.fp32_chain(R.axpby, None, src, alpha=-1.5, beta=0.0))      # one exact product
        old = _randn((n,), torch.float32, _gen(n))
        dst, check = poisoned((n,), torch.float32, device)
        dst.copy_(old)
        ops.axpby_f32_(dst, src.to(device), alpha=2.0, beta=0.5)
        check()
        R.assert_close(dst.cpu(), R.ref64(R.axpby, old, src, alpha=2.0, beta=0.5), R.fp32_chain(R.axpby, old, src, alpha=2.0, beta=0.5),
                       torch.maximum(old.double().abs(), 2 * src.double().abs()), f"axpby {name} n={n}")


@pytest.mark.parametrize("name", DT)
def test_bce_logits(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in NS + [_big_n(device)]:
        z, _, _ = _pairs(n, dtype, 300 + n)
        y = (torch.rand(n, generator=_gen(n)) < 0.4).float()
        with guarded(ops):
            loss = ops.bce_logits_fwd(z.to(device), y.to(device))
        R.assert_close(loss.cpu(), R.ref64(R.bce_logits, z, y).reshape(1), R.fp32_chain(R.bce_logits, z, y).reshape(1),
                       float(z.double().abs().max()), f"bce_fwd {name} n={n}")
        gloss = torch.tensor([0.7])
        with guarded(ops):
            dz = ops.bce_logits_bwd(z.to(device), y.to(device), gloss.to(device))
        R.assert_close(dz.cpu(), R.ref64(R.bce_logits_bwd, z, y, gloss), R.fp32_chain(R.bce_logits_bwd, z, y, gloss), 0.7 / n,
                       f"bce_bwd {name} n={n}")


@pytest.mark.parametrize("name", DT)
def test_sigmoid_bce(dvt, device, name):
    """the LSTM criterion's two kernels; a saturated logit gets the label it agrees with, so that the fp32 sigmoid's exact
    0 / 1 meets only the log term whose weight is 0 (the other one is clamped at -100 in fp32 and not in float64)"""
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in (1, 9, 257, 2051):
        z, _, _ = _pairs(n, dtype, 400 + n)
        y = (torch.rand(n, generator=_gen(n)) < 0.4).float()
        y = torch.where(z.float().abs() > 15, (z.float() > 0).float(), y)
        with guarded(ops):
            loss, prob = ops.sigmoid_bce_fwd(z.to(device), y.to(device), want_prob=True)
        R.assert_close(prob.cpu(), torch.sigmoid(z.double()), torch.sigmoid(z.float()), z.double().abs(), f"prob {name} n={n}")
        R.assert_close(loss.cpu(), R.ref64(R.sigmoid_bce, z, y).reshape(1), R.fp32_chain(R.sigmoid_bce, z, y).reshape(1),
                       float(z.double().abs().max()), f"sigmoid_bce_fwd {name} n={n}")
        gloss = torch.tensor([0.7])
        with guarded(ops):
            dz = ops.sigmoid_bce_bwd(z.to(device), y.to(device), gloss.to(device))
        R.assert_close(dz.cpu(), R.ref64(R.sigmoid_bce_bwd, z, y, gloss), R.fp32_chain(R.sigmoid_bce_bwd, z, y, gloss), 0.7 / n,
                       f"sigmoid_bce_bwd {name} n={n}")


@pytest.mark.parametrize("name", DT)
def test_ce_argmax(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for C in (1, 5, 64, 65, 400):
        for rows in (1, 3, 4, 9):
            st, te = R.ce_case(rows, C, dtype, _gen(rows * 1000 + C))
            with guarded(ops):
                loss = ops.ce_argmax_fwd(st.to(device), te.to(device))
            tag = f"{name} rows={rows} C={C}"
            R.assert_close(loss.cpu(), R.ref64(R.ce_argmax, st, te).reshape(1), R.fp32_chain(R.ce_argmax, st, te).reshape(1),
                           float(st.double().abs().max()), f"ce_argmax_fwd {tag}")
            gloss = torch.tensor([1.9])
            with guarded(ops):
                ds = ops.ce_argmax_bwd(st.to(device), te.to(device), gloss.to(device))
            R.assert_close(ds.cpu(), R.ref64(R.ce_argmax_bwd, st, te, gloss), R.fp32_chain(R.ce_argmax_bwd, st, te, gloss),
                           1.9 / rows, f"ce_argmax_bwd {tag}")


# ---------------------------------------------------------------- data movement: bitwise
@pytest.mark.parametrize("name", DT)
def test_permute_021(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for A, B, Cc in ((1, 1, 8), (3, 5, 72), (7, 2, 8), (33, 9, 512)):
        x = _randn((A, B, Cc), dtype, _gen(A * B))
        with guarded(ops):
            out = ops.permute_021(x.to(device))
        assert torch.equal(out.cpu(), x.permute(1, 0, 2).contiguous()), (A, B, Cc)


@pytest.mark.parametrize("name", DT)
def test_transpose_last2(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for B, Rr, Cc in ((1, 1, 1), (3, 33, 31), (2, 32, 64), (5, 7, 100)):
        x = _randn((B, Rr, Cc), dtype, _gen(Rr * Cc))
        with guarded(ops):
            out = ops.transpose_last2(x.to(device))
        assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous()), (B, Rr, Cc)


@pytest.mark.parametrize("path", ["vector", "scalar_cols13", "scalar_offset1"])
@pytest.mark.parametrize("name", DT)
def test_copy2d(dvt, device, name, path):
    dtype, ops = R.DTYPES[name], dvt.ops
    rows, cols, src_ld, dst_ld, off = {"vector": (5, 24, 40, 32, 0), "scalar_cols13": (5, 13, 40, 32, 0),
                                       "scalar_offset1": (5, 24, 40, 32, 1)}[path]
    src = _randn((rows * src_ld + 8,), dtype, _gen(cols + off))
    dst, check = poisoned((rows * dst_ld + 8,), dtype, device, fill=7.0)       # 7 between the rows: must stay
    ops.copy2d(src.to(device)[off:], dst[off:], rows, cols, src_ld, dst_ld)
    check()
    want = torch.full((rows * dst_ld + 8,), 7.0, dtype=dtype)
    for r in range(rows):
        want[off + r * dst_ld: off + r * dst_ld + cols] = src[off + r * src_ld: off + r * src_ld + cols]
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name", DT)
def test_rows_gather(dvt, device, name, lead):
    dtype, ops = R.DTYPES[name], dvt.ops
    for B, T, d in ((1, 1, 8), (3, 5, 72), (2, 16, 512)):
        n1 = 4                                                               # rows per source sequence: stride n1 * d > d
        src = _randn((B, T, n1, d), dtype, _gen(B * T * d))
        tok = torch.randn(d, generator=_gen(d)) if lead else None
        with guarded(ops):
            out = ops.rows_gather_fwd(src.to(device), n1 * d, None if tok is None else tok.to(device), B, T, d)
        want = R.rows_gather(src, None if tok is None else tok.to(dtype))    # (the token row is rounded once, on the way in)
        assert torch.equal(out.cpu(), want), (B, T, d)
        # backward: rows the scatter does not own keep their sentinel; dtok sums row 0 of every sequence
        dout = _randn((B, T + lead, d), dtype, _gen(B + T + d))
        for accumulate in (False, True):
            dsrc, check = poisoned((B, T, n1, d), dtype, device, fill=-3.0)
            dtok = chk2 = None
            if lead:
                dtok, chk2 = poisoned((d,), torch.float32, device, fill=5.0 if accumulate else math.nan)
            got = ops.rows_gather_bwd(dout.to(device), dsrc, n1 * d, bool(lead), B, T, d, dtok=dtok, accumulate=accumulate)
            check()
            want = torch.full((B, T, n1, d), -3.0, dtype=dtype)
            want[:, :, 0] = dout[:, lead:]
            assert torch.equal(dsrc.cpu(), want), (B, T, d, accumulate)
            if lead:
                chk2()
                assert got is dtok
                s64 = dout[:, 0].double().sum(0) + (5.0 if accumulate else 0.0)
                s32 = dout[:, 0].float().sum(0) + (5.0 if accumulate else 0.0)
                R.assert_close(dtok.cpu(), s64, s32, dout[:, 0].double().abs().max(0).values + 5.0, f"dtok {name} {B, T, d}")
            else:
                assert got is None


@pytest.mark.parametrize("name", DT)
def test_mean_rows(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for Ln in (1, 15, 16, 17, 33, 197):
        for d in (8, 72):
            for B in (1, 3):
                x = _randn((B, Ln, d), dtype, _gen(Ln * d + B))
                for scale in (None, 0.375):
                    with guarded(ops):
                        out = ops.mean_rows_fwd(x.to(device), scale)
                    R.assert_close(out.cpu(), R.ref64(R.mean_rows, x, scale=scale), R.fp32_chain(R.mean_rows, x, scale=scale),
                                   x.double().abs().max(1).values * (1.0 if scale is None else Ln * scale),
                                   f"mean_rows_fwd {name} L={Ln} d={d} B={B} scale={scale}")
    for Ln, sc in ((16, None), (4, None), (5, 0.25)):                          # a power-of-two scale: bitwise
        dout = _randn((3, 72), dtype, _gen(Ln))
        with guarded(ops):
            dx = ops.mean_rows_bwd(dout.to(device), Ln, sc)
        assert torch.equal(dx.cpu(), R.fp32_chain(R.mean_rows_bwd, dout, Ln=Ln, scale=sc, out_dtype=dtype))


@pytest.mark.parametrize("S,T", [(1, 1), (3, 1), (3, 3), (9, 3)])
@pytest.mark.parametrize("name", DT)
def test_tokens_assemble_bwd(dvt, device, name, S, T):
    dtype, ops = R.DTYPES[name], dvt.ops
    n, d = 5, 24
    dout = _randn((S, n + 1, d), dtype, _gen(S * 10 + T))
    for pos_rows in (n + 1, n + 4):
        rdemb, rdcls, rdpos = R.ref64(R.tokens_assemble_bwd, dout, T=T, pos_rows=pos_rows)
        _, cdcls, cdpos = R.fp32_chain(R.tokens_assemble_bwd, dout, T=T, pos_rows=pos_rows)
        for accumulate in (False, True):
            base = 2.0 if accumulate else 0.0
            dcls, chk1 = poisoned((d,), torch.float32, device, fill=base if accumulate else math.nan)
            dpos, chk2 = poisoned((T, pos_rows, d), torch.float32, device, fill=base if accumulate else math.nan)
            with guarded(ops):
                demb, dcls_o, dpos_o = ops.tokens_assemble_bwd(dout.to(device), T, pos_rows, dcls=dcls, dpos=dpos, accumulate=accumulate)
            chk1(); chk2()
            assert dcls_o is dcls and dpos_o is dpos
            assert torch.equal(demb.cpu(), dout[:, 1:].reshape(S * n, d))
            tag = f"{name} S={S} T={T} pos_rows={pos_rows} acc={accumulate}"
            mag_c = dout[:, 0].double().abs().max(0).values + base
            R.assert_close(dcls.cpu(), rdcls + base, cdcls + base, mag_c, f"dcls {tag}")
            R.assert_close(dpos.cpu(), rdpos + base, cdpos + base, float(dout.double().abs().max()) + base, f"dpos {tag}")
            # the surplus rows: zero when overwriting, unchanged when accumulating
            assert torch.equal(dpos.cpu()[:, n + 1:], torch.full((T, pos_rows - n - 1, d), base))
    with guarded(ops):                                                        # destinations of the wrapper's own
        demb, dcls, dpos = ops.tokens_assemble_bwd(dout.to(device), T, n + 1)
    _, rdcls, rdpos = R.ref64(R.tokens_assemble_bwd, dout, T=T, pos_rows=n + 1)
    _, cdcls, cdpos = R.fp32_chain(R.tokens_assemble_bwd, dout, T=T, pos_rows=n + 1)
    R.assert_close(dcls.cpu(), rdcls, cdcls, dout[:, 0].double().abs().max(0).values, f"dcls {name} own")
    R.assert_close(dpos.cpu(), rdpos, cdpos, float(dout.double().abs().max()), f"dpos {name} own")


@pytest.mark.parametrize("name", DT)
def test_add_rowtable(dvt, device, name):
    """small integers: every sum is exact in every dtype, so the comparison is bitwise; 7 rows with 3 rows per entry"""
    dtype, ops = R.DTYPES[name], dvt.ops
    for rows, d, rpe in ((7, 8, 3), (10, 72, 4), (1, 8, 5)):
        g = _gen(rows * d)
        x = torch.randint(-8, 9, (rows, d), generator=g).to(dtype)
        table = torch.randint(-8, 9, ((rows + rpe - 1) // rpe, d), generator=g).float()
        with guarded(ops):
            out = ops.add_rowtable(x.to(device), table.to(device), rpe)
        want = (x.float() + table[torch.arange(rows) // rpe]).to(dtype)
        assert torch.equal(out.cpu(), want), (rows, d, rpe)


# ---------------------------------------------------------------- cast / add / rows_sum: the instantiations test_gpu_ops.py leaves out
@pytest.mark.parametrize("src,dst", [("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "fp32"), ("fp16", "fp32"), ("fp32", "fp32"),
                                     ("bf16", "bf16"), ("fp16", "fp16")])
def test_cast(dvt, device, src, dst):
    ops = dvt.ops
    for n in (1, 7, 8, 9, 2051):                                            # the 8-wide body and its tail
        x = R.elementwise_values(n, R.DTYPES[src], _gen(n))
        with guarded(ops):
            out = ops.cast(x.to(device), R.DTYPES[dst])
        want = x.to(R.DTYPES[dst])
        assert out.dtype == want.dtype and torch.equal(out.cpu().view(torch.uint8), want.view(torch.uint8)), (src, dst, n)


@pytest.mark.parametrize("name", DT)
def test_add(dvt, device, name):
    dtype, ops = R.DTYPES[name], dvt.ops
    for n in (1, 7, 8, 9, 2051):
        a, b, _ = _pairs(n, dtype, 500 + n)
        with guarded(ops):
            out = ops.add(a.to(device), b.to(device))
        assert torch.equal(out.cpu(), (a.float() + b.float()).to(dtype)), (name, n)      # one fp32 sum, one rounding


@pytest.mark.parametrize("name", DT)
def test_rows_sum(dvt, device, name):
    """both kernels of ops.rows_sum: few rows of many columns (a thread per 8-column chunk), many rows (a block per chunk)"""
    dtype, ops = R.DTYPES[name], dvt.ops
    for rows, cols, stride in ((2, 8192, 8200), (16, 8192, 8192), (300, 40, 48), (17, 8, 8)):
        src = _randn((rows, stride), dtype, _gen(rows + cols))
        for accumulate in (False, True):
            out, check = poisoned((cols,), torch.float32, device, fill=1.5 if accumulate else math.nan)
            ops.rows_sum(src.to(device), stride, rows, cols, out=out, accumulate=accumulate)
            check()
            base = 1.5 if accumulate else 0.0
            R.assert_close(out.cpu(), src[:, :cols].double().sum(0) + base, src[:, :cols].float().sum(0) + base,
                           src[:, :cols].double().abs().max(0).values + base, f"rows_sum {name} {rows, cols, stride} acc={accumulate}")
