"""Exact results of every kernel of the GEMM family (dvt_gemm, dvt_gemm_pair, the split-K reduces).

Each case states the plan it expects (ops.gemm_plan: kernel, LDS-DMA configuration, K slices, tile rows, reduce) and checks
it before launching; operands come from tests/gemm_exact.py, so the output must equal a float64 product of the same
operands bit for bit (GELU: within one ulp).  C -- and aux where it is written -- is NaN inside [M, N] and canary bits in
its ldc padding and in spare rows past M, which must survive.  Operands sit at 16-byte-aligned offsets into padded
buffers.  tests/test_gemm_coverage.py ties every GEMM kernel symbol of the built library to one of these cases.
"""
import ctypes as C

import pytest
import torch

from tests import gemm_exact as X

pytestmark = pytest.mark.gpu

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": BF, "fp16": FP, "fp32": F32}
NONE, GELU, RELU, RES, DGELU, DRELU = range(6)


def P(kernel, cfg=-1, split=1, kps=None, tm=0, reduce="none", colsum="none", carry="none"):
    return dict(kernel=kernel, cfg=cfg, split=split, k_per_split=kps, tile_m=tm, reduce=reduce, colsum=colsum, carry=carry)


def G(M, N, K, ak, bk, plan, **o):
    return dict(M=M, N=N, K=K, ak=ak, bk=bk, plan=plan, **o)


# One product per case (dtype from the id's suffix).  Options: out="f32", epi, bias, alpha, acc (accumulate), colsum
# ("over" / "acc"), res32 (fp32 residual), split_k, ldpad (leading-dimension padding of the operands, 8), misalign
# (operand A starts 2 bytes off 16-byte alignment), seed.
_CASES = {
    # ---- panel-streaming kernel (launch-bound shapes)
    "small_tt32": G(264, 512, 512, True, True, P("small", tm=32), epi=NONE, bias=True),
    "small_tt64": G(1024, 512, 512, True, True, P("small", tm=64), epi=GELU, bias=True),
    "small_tf32": G(264, 512, 512, True, False, P("small", tm=32), epi=DGELU),
    "small_tf64": G(1024, 512, 512, True, False, P("small", tm=64), epi=DRELU),
    "small_ff64": G(512, 256, 264, False, False, P("small", tm=64, colsum="fused"), out="f32", colsum="over"),
    "small_ff64_acc": G(512, 256, 264, False, False, P("small", tm=64, colsum="fused"), out="f32", acc=True, colsum="acc"),
    "small_relu": G(264, 512, 512, True, True, P("small", tm=32), epi=RELU, bias=True, alpha=0.5),
    "small_res": G(264, 512, 512, True, True, P("small", tm=32), epi=RES, bias=True),
    "small_res32": G(264, 512, 512, True, True, P("small", tm=32), epi=RES, bias=True, out="f32", res32=True),
    # ---- LDS-DMA kernel: configuration 5 (256-row tiles, antiphase), every instantiated combination
    "dma5_tt_none": G(4096, 3072, 256, True, True, P("dma", cfg=5, kps=256), epi=NONE, bias=True),
    "dma5_tt_relu": G(4096, 3072, 256, True, True, P("dma", cfg=5, kps=256), epi=RELU, bias=True),
    "dma5_tt_res": G(4096, 3072, 256, True, True, P("dma", cfg=5, kps=256), epi=RES, bias=True),
    "dma5_tf_none": G(4096, 3072, 256, True, False, P("dma", cfg=5, kps=256), epi=NONE),
    "dma5_tf_drelu": G(4096, 3072, 256, True, False, P("dma", cfg=5, kps=256), epi=DRELU),
    "dma5_ff_f32": G(4096, 3072, 256, False, False, P("dma", cfg=5, kps=256), out="f32", acc=True),
    "dma5_ragged": G(4000, 3064, 256, True, True, P("dma", cfg=5, kps=256), epi=NONE),
    # split-K into slabs (16 slices of 512)
    "dma5_tt_slab": G(1024, 1024, 8192, True, True, P("dma", cfg=5, split=16, kps=512, reduce="plain")),
    "dma5_tf_slab": G(1024, 1024, 8192, True, False, P("dma", cfg=5, split=16, kps=512, reduce="plain")),
    "dma5_ff_slab": G(1024, 1024, 8192, False, False, P("dma", cfg=5, split=16, kps=512, reduce="plain", colsum="fused"),
                      out="f32", acc=True, colsum="acc"),
    # configuration 3 (16 waves): the GELU / GELU' epilogues, one slice
    "dma3_tt_gelu": G(3072, 2048, 512, True, True, P("dma", cfg=3, kps=512), epi=GELU, bias=True),
    "dma3_tf_dgelu": G(3072, 2048, 512, True, False, P("dma", cfg=3, kps=512), epi=DGELU),
    # configuration 8 (224-row tiles), ragged last tile in M and N
    "dma8_tt_none": G(3000, 2040, 512, True, True, P("dma224", cfg=8, kps=512), epi=NONE),
    "dma8_tt_res": G(3000, 2040, 512, True, True, P("dma224", cfg=8, kps=512), epi=RES, bias=True),
    "dma8_tf_none": G(3000, 2040, 512, True, False, P("dma224", cfg=8, kps=512), epi=NONE),
    # ---- 128x128 register-staged kernel
    "mfma_tt_split": G(256, 256, 2504, True, True, P("mfma128", split=14, kps=192, reduce="plain")),
    "mfma_tf_res": G(3000, 2040, 512, True, False, P("mfma128", kps=512), epi=RES, bias=True),      # cfg 8 -> 5 -> none
    "mfma_ft": G(2048, 1024, 1024, False, True, P("mfma128", split=2, kps=512, reduce="epilogue"), epi=RELU, bias=True),
    "mfma_tt_f32": G(3072, 2048, 512, True, True, P("mfma128", kps=512), out="f32", bias=True, acc=True),
    "mfma_ff_ragged": G(256, 256, 2501, False, False, P("mfma128", split=14, kps=192, reduce="plain"), out="f32"),
    "mfma_ft_split": G(256, 256, 512, False, True, P("mfma128", split=4, kps=128, reduce="plain")),
    "mfma_epi_gelu": G(256, 256, 2504, True, True, P("mfma128", split=14, kps=192, reduce="epilogue"), epi=GELU, bias=True),
    "mfma_epi_relu": G(256, 256, 2504, True, True, P("mfma128", split=14, kps=192, reduce="epilogue"), epi=RELU, bias=True,
                       alpha=2.0),
    "mfma_epi_res": G(256, 256, 2504, True, True, P("mfma128", split=14, kps=192, reduce="epilogue"), epi=RES, bias=True),
    "mfma_epi_dgelu": G(256, 256, 2504, True, False, P("mfma128", split=14, kps=192, reduce="epilogue"), epi=DGELU),
    "mfma_epi_drelu": G(256, 256, 2504, True, False, P("mfma128", split=14, kps=192, reduce="epilogue"), epi=DRELU,
                        alpha=0.5),
    "mfma_epi_f32": G(256, 256, 2504, True, True, P("mfma128", split=14, kps=192, reduce="epilogue"), out="f32", bias=True,
                      acc=True),
    # ---- generic route: 16-bit products the MFMA kernels refuse, and fp32
    "gen64_n300": G(200, 300, 100, True, True, P("generic64"), epi=RELU, bias=True),
    "gen64_res": G(200, 299, 96, True, False, P("generic64"), epi=RES, bias=True),
    "gen64_dgelu": G(200, 304, 100, True, False, P("generic64"), epi=DGELU),                  # K % 8, k-major A
    "gen64_drelu": G(200, 304, 96, True, True, P("generic64"), epi=DRELU, ldpad=3),          # lda % 8
    "gen64_gelu": G(200, 304, 96, True, True, P("generic64"), epi=GELU, bias=True, misalign=True),
    "gen64_colsum": G(200, 299, 96, False, False, P("generic64", colsum="alone"), out="f32", acc=True, colsum="acc",
                      alpha=0.5),
    "tinyw": G(8, 19, 512, True, True, P("tiny_wave"), epi=NONE, bias=True),
    "tinyw_f32acc": G(19, 512, 264, False, False, P("tiny_wave", colsum="alone"), out="f32", acc=True, colsum="over"),
    "tinyt": G(100, 200, 32, True, True, P("tiny_thread"), epi=RES, bias=True, ldpad=1),
    "tinyt_drelu": G(100, 199, 24, True, False, P("tiny_thread"), epi=DRELU, alpha=2.0),
}
_DT16 = ("bf16", "fp16")
CASES = {}
for _k, _v in _CASES.items():
    for _d in _DT16:
        CASES[f"{_k}-{_d}"] = dict(_v, dtype=DTYPES[_d])
# fp32 mode (every fp32 product is generic)
for _k in ("gen64_n300", "gen64_res", "gen64_colsum", "tinyw", "tinyw_f32acc", "tinyt", "tinyt_drelu"):
    _v = dict(_CASES[_k], dtype=F32)
    _v.pop("out", None)
    CASES[f"{_k}-fp32"] = _v


def _gelu_alpha(M, N, K, seed):
    """power of two that keeps |alpha * acc| <= 2.5 (the GELU pre-activation then lies in [-3.5, 3.5] with bias in -1..1)"""
    A, B = X.operands(M, N, K, seed)
    m = float((A @ B).abs().max())
    a = 1.0
    while a * m > 2.5:
        a /= 2
    return a


def build(cid, device, fill=True):
    """-> (kwargs of ops.gemm, context for the check).  fill=False: shapes, strides and alignment only (plan queries)."""
    c = CASES[cid]
    M, N, K, ak, bk, dtype = c["M"], c["N"], c["K"], c["ak"], c["bk"], c["dtype"]
    epi = c.get("epi", NONE)
    seed = c.get("seed", M * 7 + N * 3 + K)
    out_dtype = F32 if c.get("out") == "f32" or dtype == F32 else dtype
    alpha = c.get("alpha", 1.0)
    if epi == GELU:
        alpha = min(alpha, _gelu_alpha(M, N, K, seed)) if fill else 0.125
    if fill:
        A, B = X.operands(M, N, K, seed)
    else:
        A, B = torch.zeros(M, K, dtype=torch.float64), torch.zeros(K, N, dtype=torch.float64)
    pad = c.get("ldpad", 8)
    off = 1 if c.get("misalign") else 8
    Av, lda = X.layout(A if ak else A.t(), ak, dtype, device, pad=pad, offset=off)
    Bv, ldb = X.layout(B.t() if bk else B, bk, dtype, device, pad=pad)
    ctx = dict(A=A, B=B, Av=Av, Bv=Bv, M=M, N=N, K=K, epi=epi, alpha=alpha, out_dtype=out_dtype, dtype=dtype)
    kw = dict(a_kmajor=ak, b_kmajor=bk, lda=lda, ldb=ldb, epilogue=epi, alpha=alpha, out_dtype=out_dtype,
              split_k=c.get("split_k", 0))
    if c.get("bias"):
        bias = X.small_ints((N,), -1 if epi == GELU else -3, 1 if epi == GELU else 3, seed + 2) if fill else torch.zeros(N)
        kw["bias"] = bias.float().to(device)
        ctx["bias"] = bias
    if epi == RES:
        rdt = F32 if c.get("res32") else dtype
        res = X.small_ints((M, N), -8, 8, seed + 3) if fill else torch.zeros(M, N, dtype=torch.float64)
        rbuf = torch.zeros(M, N + 8, dtype=rdt, device=device)
        rbuf[:, :N] = res.to(rdt)
        kw["residual"] = rbuf[:, :N]
        ctx["residual"] = res
    if epi in (DGELU, DRELU, GELU):
        abuf, aview = X.canaried(M, N, dtype, device)
        if epi == DGELU:
            aux = X.grid16((M, N), dtype, seed + 4) if fill else torch.zeros(M, N, dtype=torch.float64)
        elif epi == DRELU:
            aux = X.small_ints((M, N), -1, 1, seed + 4) if fill else torch.zeros(M, N, dtype=torch.float64)
        if epi != GELU:
            aview.copy_(aux.to(dtype))
            ctx["aux"] = aux
        kw["aux"] = aview
        ctx["aux_buf"] = abuf
    prior = None
    if c.get("acc"):
        prior = X.small_ints((M, N), -50, 50, seed + 5) if fill else None
        kw["accumulate"] = True
    cbuf, cview = X.canaried(M, N, out_dtype, device, fill=prior)
    kw["out"] = cview
    ctx["prior"], ctx["C_buf"] = prior, cbuf
    if c.get("colsum"):
        cs_prior = X.small_ints((M,), -20, 20, seed + 6) if fill else torch.zeros(M, dtype=torch.float64)
        cs = torch.full((M + 8,), float("nan"), dtype=F32, device=device)
        if c["colsum"] == "acc":
            cs[:M] = cs_prior.float()
            kw["colsum_accumulate"] = True
        kw["colsum_out"] = cs[:M]
        ctx["colsum"], ctx["cs_prior"] = cs, (cs_prior if c["colsum"] == "acc" else None)
    return kw, ctx


def instantiation(p, ak, bk, epi, out_f32):
    """the plan fields naming the launched instantiation: layouts, epilogue (the reduce's with LDS-DMA slabs), output form"""
    slab = p["split"] > 1
    return dict(p, a_kmajor=ak, b_kmajor=bk, out="slab" if slab else "f32" if out_f32 else "in",
                epilogue=NONE if slab and p["kernel"] != "mfma128" else epi)


def expected_plan(cid):
    c = CASES[cid]
    p = dict(c["plan"])
    if p["k_per_split"] is None:
        p["k_per_split"] = -(-c["K"] // 64) * 64 if p["kernel"] in ("dma", "dma224", "mfma128") else 0
    from dvt_amd import ops
    return ops.GemmPlan(**instantiation(p, c["ak"], c["bk"], c.get("epi", NONE), c.get("out") == "f32" or c["dtype"] == F32))


def reference(ctx):
    """float64 C (rounded once to the output type where the epilogue multiplies) and the GELU pre-activation"""
    A, B = ctx["A"], ctx["B"]
    acc = (A.cuda() @ B.cuda()).cpu()
    check_dtype = ctx["out_dtype"]
    if ctx["epi"] not in (GELU, DGELU):
        X.check_bound(acc * ctx["alpha"], check_dtype)
    ref, pre = X.epilogue64(acc, ctx["epi"], alpha=ctx["alpha"], bias=ctx.get("bias"), residual=ctx.get("residual"),
                            aux=ctx.get("aux"))
    if ctx["prior"] is not None:
        ref = ref + ctx["prior"]
    if ctx["epi"] != GELU:
        if ctx["epi"] == DGELU:
            ref = ref.to(check_dtype).double()        # the one rounding of an exact product
        X.check_bound(ref, check_dtype)
    return ref, pre


def verify(ctx, label=""):
    M, N = ctx["M"], ctx["N"]
    ref, pre = reference(ctx)
    got = ctx["C_buf"][:M, :N].double().cpu()
    if ctx["epi"] == GELU:
        tol = X.ulp(ref, ctx["out_dtype"])
        bad = ((got - ref).abs() > tol) | got.isnan()
        assert not bad.any(), f"{label}GELU: {int(bad.sum())} outputs beyond one ulp, first {bad.nonzero()[:4].tolist()}"
        if ctx.get("aux_buf") is not None:
            g = ctx["aux_buf"][:M, :N].double().cpu()
            rg = X.gelu_grad64(pre)
            badg = ((g - rg).abs() > X.ulp(rg, ctx["dtype"])) | g.isnan()
            assert not badg.any(), f"{label}GELU': {int(badg.sum())} derivatives beyond one ulp, first {badg.nonzero()[:4].tolist()}"
    else:
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), (f"{label}{bad.shape[0]} outputs differ, first {bad[:4].tolist()}: "
                                       f"{got[tuple(bad[0])]} != {ref[tuple(bad[0])]}")
    n = X.canaries_intact(ctx["C_buf"], M, N)
    assert n == 0, f"{label}{n} elements of C outside [M, N] overwritten"
    if ctx.get("aux_buf") is not None:
        n = X.canaries_intact(ctx["aux_buf"], M, N)
        assert n == 0, f"{label}{n} elements of aux outside [M, N] overwritten"
        if ctx["epi"] in (DGELU, DRELU):
            assert torch.equal(ctx["aux_buf"][:M, :N].double().cpu(), ctx["aux"]), f"{label}aux was written"
    if ctx.get("colsum") is not None:
        cs = ctx["colsum"].double().cpu()
        want = ctx["A"].sum(1) + (ctx["cs_prior"] if ctx["cs_prior"] is not None else 0)
        assert torch.equal(cs[:M], want), f"{label}colsum_out differs at {int((cs[:M] != want).sum())} rows"
        assert cs[M:].isnan().all(), f"{label}colsum_out written past M"


def run(cid, device):
    """plan check, launch, exact check of one case"""
    from dvt_amd import ops
    c = CASES[cid]
    kw, ctx = build(cid, device)
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], c["M"], c["N"], c["K"], **kw) == expected_plan(cid)
    ops.gemm(ctx["Av"], ctx["Bv"], c["M"], c["N"], c["K"], **kw)
    torch.cuda.synchronize()
    verify(ctx)


@pytest.mark.parametrize("cid", list(CASES))
def test_gemm_exact(device, cid):
    run(cid, device)


def _desc_of(cid, device):
    from dvt_amd import ops
    c = CASES[cid]
    kw, ctx = build(cid, device)
    d, _ = ops._gemm_desc(ctx["Av"], ctx["Bv"], c["M"], c["N"], c["K"], **kw)
    return d, ctx


@pytest.mark.parametrize("dname", list(_DT16))
def test_gemm_split_without_workspace(device, dname):
    """A planned split with no workspace (only through the C ABI: ops.gemm always passes one) runs unsplit on the 128x128
    kernel -- the plan says so and the result is exact."""
    import dvt_amd
    from dvt_amd import ops
    lib = dvt_amd._lib.load()
    d, ctx = _desc_of(f"mfma_epi_relu-{dname}", device)
    q = dvt_amd._lib.GemmPlanInfo()
    d.workspace = 256
    assert lib.dvt_gemm_plan(C.byref(d), C.byref(q)) == 0 and ops._plan_tuple(q).split == 14
    d.workspace = None
    assert lib.dvt_gemm_plan(C.byref(d), C.byref(q)) == 0
    assert ops._plan_tuple(q) == ops.GemmPlan("mfma128", -1, 1, 2560, epilogue=RELU)
    dvt_amd._lib.check(lib.dvt_gemm(C.byref(d), ops._stream()), "dvt_gemm")
    torch.cuda.synchronize()
    verify(ctx)


@pytest.mark.parametrize("size", ["64", "32"])
@pytest.mark.parametrize("dname", list(_DT16))
def test_gemm_pair_exact(device, dname, size):
    """dvt_gemm_pair as one launch (gemm_small_pair_kernel, data-gradient tiles of 32 or 64 rows): exact against float64
    and equal to the two products launched one after the other."""
    import dvt_amd
    from dvt_amd import ops
    lib = dvt_amd._lib.load()
    dtype = DTYPES[dname]
    T = 264 if size == "32" else 1024                 # rows of dy; dW = dy^T x [N, K], dx = dy w [T, K]
    N, K = 256, 512
    dy = X.sparse_rows(N, T, seed=T).t().contiguous()          # [T, N]: sparse along T (the reduction of dW)
    xx = X.dense(T, K, seed=T + 1)                              # [T, K]
    w = X.sparse_rows(K, N, seed=T + 2).t().contiguous()        # [N, K]: sparse along N (the reduction of dx)
    dyv, ld_dy = X.layout(dy, False, dtype, device)
    xv, ld_x = X.layout(xx, False, dtype, device)
    wv, ld_w = X.layout(w, False, dtype, device)
    outs = []
    for fused in (True, False):
        wbuf, wview = X.canaried(N, K, F32, device)
        cs = torch.full((N + 8,), float("nan"), dtype=F32, device=device)
        gbuf, gview = X.canaried(T, K, dtype, device)
        wk = dict(A=dyv, B=xv, M=N, N=K, K=T, a_kmajor=False, b_kmajor=False, lda=ld_dy, ldb=ld_x, out=wview,
                  out_dtype=F32, colsum_out=cs[:N])
        gk = dict(A=dyv, B=wv, M=T, N=K, K=N, a_kmajor=True, b_kmajor=False, lda=ld_dy, ldb=ld_w, out=gview)
        tm = 32 if size == "32" else 64
        if fused:
            assert ops.gemm_pair_plan(wk, gk) == (ops.GemmPlan("small_pair", tile_m=64, colsum="fused", a_kmajor=False,
                                                               b_kmajor=False, out="f32"),
                                                  ops.GemmPlan("small_pair", tile_m=tm, b_kmajor=False))
            wd, _ = ops._gemm_desc(**wk)
            gd, _ = ops._gemm_desc(**gk)
            assert lib.dvt_gemm_pair_fused(C.byref(wd), C.byref(gd)) == 1
            dvt_amd._lib.check(lib.dvt_gemm_pair(C.byref(wd), C.byref(gd), ops._stream()), "dvt_gemm_pair")
        else:
            ops.gemm(**wk)
            ops.gemm(**gk)
        torch.cuda.synchronize()
        rw = (dy.t().cuda() @ xx.cuda()).cpu()
        rg = (dy.cuda() @ w.cuda()).cpu()
        X.check_bound(rw, dtype)
        X.check_bound(rg, dtype)
        assert torch.equal(wview.double().cpu(), rw) and torch.equal(gview.double().cpu(), rg), f"fused={fused}"
        assert torch.equal(cs[:N].double().cpu(), dy.sum(0)) and cs[N:].isnan().all()
        assert X.canaries_intact(wbuf, N, K) == 0 and X.canaries_intact(gbuf, T, K) == 0
        outs.append((wbuf.clone(), gbuf.clone(), cs.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# deferred weight gradients: (M, N, K) of the deferring product, its plan, the carrying call's case id and what it does with
# the carried reduce
CARRY_CASES = {
    "tail": ((1024, 1024, 8192), P("dma", cfg=5, split=16, kps=512, reduce="deferred", colsum="fused"), "dma5_tf_none",
             "tail"),
    "alone": ((1024, 1024, 8192), P("dma", cfg=5, split=16, kps=512, reduce="deferred", colsum="fused"), "small_tf32",
              "alone"),
    "wide": ((512, 256, 32768), P("dma", cfg=5, split=64, kps=512, reduce="deferred"), "small_tf32", "wide"),
}


@pytest.mark.parametrize("dname", list(_DT16))
@pytest.mark.parametrize("how", list(CARRY_CASES))
def test_gemm_deferred_reduce_exact(device, how, dname):
    """A weight gradient whose split-K reduce is deferred and then performed by the next call: in the grid tail of a
    one-slice LDS-DMA launch, or on its own first (splitk_reduce_kernel; splitk_reduce_wide_kernel for >= 64 slices of a
    small product).  Both products exact, both sets of canaries intact."""
    from dvt_amd import ops
    dtype = DTYPES[dname]
    (M, N, K), plan, carrier, carry = CARRY_CASES[how]
    A = X.sparse_rows(M, K, seed=M + K).double()
    B = X.dense(N, K, seed=N + K).t()
    Av, lda = X.layout(A.t(), False, dtype, device)
    Bv, ldb = X.layout(B, False, dtype, device)
    prior = X.small_ints((M, N), -50, 50, seed=3)
    cbuf, cview = X.canaried(M, N, F32, device, fill=prior)
    cs = None
    kw = dict(a_kmajor=False, b_kmajor=False, lda=lda, ldb=ldb, out=cview, out_dtype=F32, accumulate=True)
    if plan["colsum"] != "none":
        cs = torch.full((M + 8,), float("nan"), dtype=F32, device=device)
        kw["colsum_out"] = cs[:M]
    assert ops.gemm_plan(Av, Bv, M, N, K, defer_reduce=True, **kw) == ops.GemmPlan(**instantiation(plan, False, False, NONE, True))
    _, pending = ops.gemm(Av, Bv, M, N, K, defer_reduce=True, **kw)
    assert pending.valid == 1 and pending.splits == plan["split"]
    c = CASES[f"{carrier}-{dname}"]
    ckw, cctx = build(f"{carrier}-{dname}", device)
    exp = expected_plan(f"{carrier}-{dname}")._replace(carry=carry)
    assert ops.gemm_plan(cctx["Av"], cctx["Bv"], c["M"], c["N"], c["K"], carry=pending, **ckw) == exp
    ops.gemm(cctx["Av"], cctx["Bv"], c["M"], c["N"], c["K"], carry=pending, **ckw)
    pending.valid = 0                                  # performed by that call
    torch.cuda.synchronize()
    verify(cctx, "carrying call: ")
    ref = (A.cuda() @ B.cuda()).cpu()
    X.check_bound(ref, dtype)
    got = cview.double().cpu()
    assert torch.equal(got, ref + prior), f"deferred product: {int((got != ref + prior).sum())} outputs differ"
    assert X.canaries_intact(cbuf, M, N) == 0
    if cs is not None:
        assert torch.equal(cs[:M].double().cpu(), A.sum(1)) and cs[M:].isnan().all()


GENERIC_FP32 = {"generic64": (200, 300, 100), "tiny_wave": (8, 19, 512), "tiny_thread": (100, 200, 32)}


@pytest.mark.parametrize("kernel", list(GENERIC_FP32))
def test_fp32_mode_within_one_ulp(device, kernel):
    """fp32 mode accumulates in double (gemm_generic_kernel, gemm_tiny_kernel): random fp32 operands give the float64
    product rounded once -- within one fp32 ulp of it at every output."""
    from dvt_amd import ops
    M, N, K = GENERIC_FP32[kernel]
    g = torch.Generator().manual_seed(K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g)
    Av, Bv = A.to(device), B.to(device)
    assert ops.gemm_plan(Av, Bv, M, N, K, a_kmajor=True, b_kmajor=True, lda=K, ldb=K) == ops.GemmPlan(kernel, out="f32")
    got = ops.gemm(Av, Bv, M, N, K, a_kmajor=True, b_kmajor=True, lda=K, ldb=K).double().cpu()
    ref = A.double() @ B.double().t()
    err = (got - ref).abs()
    tol = X.ulp(ref, F32)
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {M * N} outputs beyond one ulp, worst {float((err / tol).max()):.2f} ulp"
