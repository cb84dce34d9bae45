"""CPU gate on the GEMM family's exact tests: every GEMM kernel symbol of the built library is either launched by a named
case of tests/test_gpu_gemm_exact.py -- the library's own plan query (dvt_gemm_plan) says that case takes that
instantiation -- or listed as unreachable from dvt_gemm with a reason; and the operands of those cases see a missing,
doubled or misplaced k-step and a misplaced output fragment.

The convolution forms of the LDS-DMA kernel (gemm_dma_kernel<..., true>: the A operand gathered from an NHWC map) are not
this gate's: tests/test_conv_coverage.py accounts for every one of them, with tests/test_gpu_conv_exact.py."""
import re

import pytest
import torch

from tests import gemm_exact as X

# every GEMM kernel symbol -> the exact GPU case that launches it
GEMM_COVERAGE = {
    "gemm_dma_kernel<std::bfloat16_t, true, true, 5, 0, 0, false>": "test_gemm_exact[dma5_tt_none-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 5, 2, 0, false>": "test_gemm_exact[dma5_tt_relu-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 5, 3, 0, false>": "test_gemm_exact[dma5_tt_res-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, false, 5, 0, 0, false>": "test_gemm_exact[dma5_tf_none-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, false, 5, 5, 0, false>": "test_gemm_exact[dma5_tf_drelu-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, false, false, 5, 0, 1, false>": "test_gemm_exact[dma5_ff_f32-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 5, 0, 2, false>": "test_gemm_exact[dma5_tt_slab-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, false, 5, 0, 2, false>": "test_gemm_exact[dma5_tf_slab-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, false, false, 5, 0, 2, false>": "test_gemm_exact[dma5_ff_slab-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 3, 1, 0, false>": "test_gemm_exact[dma3_tt_gelu-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, false, 3, 4, 0, false>": "test_gemm_exact[dma3_tf_dgelu-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 8, 0, 0, false>": "test_gemm_exact[dma8_tt_none-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, true, 8, 3, 0, false>": "test_gemm_exact[dma8_tt_res-bf16]",
    "gemm_dma_kernel<std::bfloat16_t, true, false, 8, 0, 0, false>": "test_gemm_exact[dma8_tf_none-bf16]",
    "gemm_mfma_kernel<std::bfloat16_t, true, true>": "test_gemm_exact[mfma_tt_split-bf16]",
    "gemm_mfma_kernel<std::bfloat16_t, true, false>": "test_gemm_exact[mfma_tf_res-bf16]",
    "gemm_mfma_kernel<std::bfloat16_t, false, true>": "test_gemm_exact[mfma_ft-bf16]",
    "gemm_mfma_kernel<std::bfloat16_t, false, false>": "test_gemm_exact[mfma_ff_ragged-bf16]",
    "gemm_small_kernel<std::bfloat16_t, true, true, 32>": "test_gemm_exact[small_tt32-bf16]",
    "gemm_small_kernel<std::bfloat16_t, true, true, 64>": "test_gemm_exact[small_tt64-bf16]",
    "gemm_small_kernel<std::bfloat16_t, true, false, 32>": "test_gemm_exact[small_tf32-bf16]",
    "gemm_small_kernel<std::bfloat16_t, true, false, 64>": "test_gemm_exact[small_tf64-bf16]",
    "gemm_small_kernel<std::bfloat16_t, false, false, 64>": "test_gemm_exact[small_ff64-bf16]",
    "gemm_small_pair_kernel<std::bfloat16_t, 32>": "test_gemm_pair_exact[bf16-32]",
    "gemm_small_pair_kernel<std::bfloat16_t, 64>": "test_gemm_pair_exact[bf16-64]",
    "gemm_dma_kernel<_Float16, true, true, 5, 0, 0, false>": "test_gemm_exact[dma5_tt_none-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 5, 2, 0, false>": "test_gemm_exact[dma5_tt_relu-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 5, 3, 0, false>": "test_gemm_exact[dma5_tt_res-fp16]",
    "gemm_dma_kernel<_Float16, true, false, 5, 0, 0, false>": "test_gemm_exact[dma5_tf_none-fp16]",
    "gemm_dma_kernel<_Float16, true, false, 5, 5, 0, false>": "test_gemm_exact[dma5_tf_drelu-fp16]",
    "gemm_dma_kernel<_Float16, false, false, 5, 0, 1, false>": "test_gemm_exact[dma5_ff_f32-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 5, 0, 2, false>": "test_gemm_exact[dma5_tt_slab-fp16]",
    "gemm_dma_kernel<_Float16, true, false, 5, 0, 2, false>": "test_gemm_exact[dma5_tf_slab-fp16]",
    "gemm_dma_kernel<_Float16, false, false, 5, 0, 2, false>": "test_gemm_exact[dma5_ff_slab-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 3, 1, 0, false>": "test_gemm_exact[dma3_tt_gelu-fp16]",
    "gemm_dma_kernel<_Float16, true, false, 3, 4, 0, false>": "test_gemm_exact[dma3_tf_dgelu-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 8, 0, 0, false>": "test_gemm_exact[dma8_tt_none-fp16]",
    "gemm_dma_kernel<_Float16, true, true, 8, 3, 0, false>": "test_gemm_exact[dma8_tt_res-fp16]",
    "gemm_dma_kernel<_Float16, true, false, 8, 0, 0, false>": "test_gemm_exact[dma8_tf_none-fp16]",
    "gemm_mfma_kernel<_Float16, true, true>": "test_gemm_exact[mfma_tt_split-fp16]",
    "gemm_mfma_kernel<_Float16, true, false>": "test_gemm_exact[mfma_tf_res-fp16]",
    "gemm_mfma_kernel<_Float16, false, true>": "test_gemm_exact[mfma_ft-fp16]",
    "gemm_mfma_kernel<_Float16, false, false>": "test_gemm_exact[mfma_ff_ragged-fp16]",
    "gemm_small_kernel<_Float16, true, true, 32>": "test_gemm_exact[small_tt32-fp16]",
    "gemm_small_kernel<_Float16, true, true, 64>": "test_gemm_exact[small_tt64-fp16]",
    "gemm_small_kernel<_Float16, true, false, 32>": "test_gemm_exact[small_tf32-fp16]",
    "gemm_small_kernel<_Float16, true, false, 64>": "test_gemm_exact[small_tf64-fp16]",
    "gemm_small_kernel<_Float16, false, false, 64>": "test_gemm_exact[small_ff64-fp16]",
    "gemm_small_pair_kernel<_Float16, 32>": "test_gemm_pair_exact[fp16-32]",
    "gemm_small_pair_kernel<_Float16, 64>": "test_gemm_pair_exact[fp16-64]",
    "gemm_generic_kernel<std::bfloat16_t>": "test_gemm_exact[gen64_n300-bf16]",
    "gemm_tiny_kernel<std::bfloat16_t, true>": "test_gemm_exact[tinyw-bf16]",
    "gemm_tiny_kernel<std::bfloat16_t, false>": "test_gemm_exact[tinyt-bf16]",
    "gemm_generic_kernel<_Float16>": "test_gemm_exact[gen64_n300-fp16]",
    "gemm_tiny_kernel<_Float16, true>": "test_gemm_exact[tinyw-fp16]",
    "gemm_tiny_kernel<_Float16, false>": "test_gemm_exact[tinyt-fp16]",
    "gemm_generic_kernel<float>": "test_gemm_exact[gen64_n300-fp32]",
    "gemm_tiny_kernel<float, true>": "test_gemm_exact[tinyw-fp32]",
    "gemm_tiny_kernel<float, false>": "test_gemm_exact[tinyt-fp32]",
    "splitk_reduce_kernel<float>": "test_gemm_exact[dma5_ff_slab-bf16]",
    "splitk_reduce_kernel<std::bfloat16_t>": "test_gemm_exact[dma5_tt_slab-bf16]",
    "splitk_reduce_kernel<_Float16>": "test_gemm_exact[dma5_tt_slab-fp16]",
    "splitk_reduce_epi_kernel<std::bfloat16_t>": "test_gemm_exact[mfma_epi_gelu-bf16]",
    "splitk_reduce_epi_kernel<_Float16>": "test_gemm_exact[mfma_epi_gelu-fp16]",
    "splitk_reduce_wide_kernel": "test_gemm_deferred_reduce_exact[wide-bf16]",
}

_E = {"std::bfloat16_t": "bf16", "_Float16": "fp16", "float": "fp32"}
_T = {"bf16": "std::bfloat16_t", "fp16": "_Float16", "fp32": "float"}


def _unreachable():
    """plain-GEMM instantiations dvt_gemm never launches (tools/gemm_bench.hip and tools/dev/ may): plan_gemm picks only
    configurations 3 (GELU / GELU' epilogues, one slice), 5 and 8, and 5 never with those two epilogues"""
    why0 = "plan_gemm never picks LDS-DMA configuration 0 (5 replaced it)"
    why1 = "plan_gemm never picks LDS-DMA configuration 1 (it serves convolutions)"
    why3 = "plan_gemm picks configuration 3 only for the GELU / GELU' epilogues with one slice"
    why5 = "plan_gemm picks configuration 3, not 5, for the GELU / GELU' epilogues"
    combos = [(True, True, e, 0) for e in (0, 1, 2, 3)] + [(True, False, e, 0) for e in (0, 4, 5)] + \
             [(False, False, 0, 1)] + [(True, True, 0, 2), (True, False, 0, 2), (False, False, 0, 2)]
    out = {}
    for e in ("std::bfloat16_t", "_Float16"):
        for ak, bk, epi, o in combos:
            args = f"{str(ak).lower()}, {str(bk).lower()}"
            if e == "std::bfloat16_t":
                out[f"gemm_dma_kernel<{e}, {args}, 1, {epi}, {o}, false>"] = why1
            out[f"gemm_dma_kernel<{e}, {args}, 0, {epi}, {o}, false>"] = why0
            if not ((ak, bk, epi, o) in ((True, True, 1, 0), (True, False, 4, 0))):
                out[f"gemm_dma_kernel<{e}, {args}, 3, {epi}, {o}, false>"] = why3
            else:
                out[f"gemm_dma_kernel<{e}, {args}, 5, {epi}, {o}, false>"] = why5
    return out


UNREACHABLE = _unreachable()

_FAMILY = re.compile(r"^(gemm_dma_kernel<.*, false>|gemm_mfma_kernel<.*>|gemm_small_kernel<.*>|gemm_small_pair_kernel<.*>|"
                     r"gemm_generic_kernel<.*>|gemm_tiny_kernel<.*>|splitk_reduce_kernel<.*>|splitk_reduce_epi_kernel<.*>|"
                     r"splitk_reduce_wide_kernel)$")


def _short(sym):
    s = sym.replace("(anonymous namespace)::", "")
    if s.startswith("void "):
        s = s[len("void "):]
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(s[i], 0)
            if depth == 0:
                return s[:i]
    return s


@pytest.fixture(scope="module")
def gemm_symbols():
    import os
    import sys
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        from isa_listing import kernel_listings
    finally:
        sys.path.pop(0)
    return {_short(s) for s in kernel_listings(dvt_amd._lib.LIB_PATH, demangle=True) if _FAMILY.match(_short(s))}


def _b(x):
    return "true" if x else "false"


def symbols_of(plan, e, out_f32):
    """the kernel symbols a dvt_gemm call with this plan launches (e: element type of the operands; out_f32: of C)"""
    ak, bk, epi = plan.a_kmajor, plan.b_kmajor, plan.epilogue
    o = {"in": 0, "f32": 1, "slab": 2}[plan.out]
    oute = "float" if out_f32 else e
    k = plan.kernel
    out = set()
    if k in ("dma", "dma224"):
        out.add(f"gemm_dma_kernel<{e}, {_b(ak)}, {_b(bk)}, {plan.cfg}, {epi}, {o}, false>")
    elif k == "mfma128":
        out.add(f"gemm_mfma_kernel<{e}, {_b(ak)}, {_b(bk)}>")
    elif k == "small":
        out.add(f"gemm_small_kernel<{e}, {_b(ak)}, {_b(bk)}, {plan.tile_m}>")
    elif k == "generic64":
        out.add(f"gemm_generic_kernel<{e}>")
    elif k in ("tiny_wave", "tiny_thread"):
        out.add(f"gemm_tiny_kernel<{e}, {_b(k == 'tiny_wave')}>")
    if plan.reduce == "plain":                      # (slabs of a 16-bit output are summed into the 16-bit type)
        out.add(f"splitk_reduce_kernel<{oute}>")
    elif plan.reduce == "epilogue":
        out.add(f"splitk_reduce_epi_kernel<{e}>")
    if plan.carry == "alone":
        out.add("splitk_reduce_kernel<float>")
    elif plan.carry == "wide":
        out.add("splitk_reduce_wide_kernel")
    return out


def _case_symbols(case):
    """the symbols a named GPU case launches, from the library's plan query at 256 CUs (no device)"""
    from dvt_amd import ops
    from tests import test_gpu_gemm_exact as G
    fn, params = re.match(r"^(\w+)\[(.+)\]$", case).groups()
    assert hasattr(G, fn), case
    if fn == "test_gemm_exact":
        assert params in G.CASES, case
        c = G.CASES[params]
        kw, ctx = G.build(params, "cpu", fill=False)
        plan = ops.gemm_plan(ctx["Av"], ctx["Bv"], c["M"], c["N"], c["K"], **kw)
        assert plan == G.expected_plan(params), case
        return symbols_of(plan, _T[params.rsplit("-", 1)[1]], kw["out_dtype"] == torch.float32)
    if fn == "test_gemm_pair_exact":
        dname, size = params.split("-")
        assert dname in G.DTYPES and size in ("32", "64"), case
        T, N, K, dt = (264 if size == "32" else 1024), 256, 512, G.DTYPES[dname]
        dy, x, w = torch.empty(T, N, dtype=dt), torch.empty(T, K, dtype=dt), torch.empty(N, K, dtype=dt)
        pw, pg = ops.gemm_pair_plan(dict(A=dy, B=x, M=N, N=K, K=T, a_kmajor=False, b_kmajor=False, lda=N, ldb=K,
                                         out_dtype=torch.float32),
                                    dict(A=dy, B=w, M=T, N=K, K=N, a_kmajor=True, b_kmajor=False, lda=N, ldb=K))
        assert pw.kernel == pg.kernel == "small_pair" and pw.tile_m == 64, case
        return {f"gemm_small_pair_kernel<{_T[dname]}, {pg.tile_m}>"}
    if fn == "test_gemm_deferred_reduce_exact":
        how, dname = params.split("-")
        (M, N, K), plan, carrier, carry = G.CARRY_CASES[how]
        dt = G.DTYPES[dname]
        A, B = torch.empty(K, M, dtype=dt), torch.empty(K, N, dtype=dt)
        kw = dict(a_kmajor=False, b_kmajor=False, lda=M, ldb=N, out_dtype=torch.float32)
        if plan["colsum"] != "none":
            kw["colsum_out"] = torch.empty(M)
        pd = ops.gemm_plan(A, B, M, N, K, defer_reduce=True, **kw)
        assert pd == ops.GemmPlan(**G.instantiation(plan, False, False, 0, True)), case
        out = symbols_of(pd, _T[dname], True)
        cid = f"{carrier}-{dname}"
        c = G.CASES[cid]
        ckw, ctx = G.build(cid, "cpu", fill=False)
        pend = __import__("dvt_amd")._lib.SplitKPending(valid=1, splits=pd.split, M=M, N=N, C=256, ldc=N, slab=256,
                                                       cs_slab=256 if plan["colsum"] != "none" else None)
        pc = ops.gemm_plan(ctx["Av"], ctx["Bv"], c["M"], c["N"], c["K"], carry=pend, **ckw)
        assert pc.carry == carry, case
        return out | symbols_of(pc, _T[dname], ckw["out_dtype"] == torch.float32)
    raise AssertionError(f"unknown case {case}")


def test_every_gemm_kernel_has_an_exact_gpu_case(gemm_symbols):
    assert len(gemm_symbols) > 60, "the listing has (almost) no GEMM kernels: the disassembly found nothing"
    missing = gemm_symbols - set(GEMM_COVERAGE) - set(UNREACHABLE)
    assert not missing, f"GEMM kernels without an exact GPU case in GEMM_COVERAGE (or a reason in UNREACHABLE): {sorted(missing)}"
    stale = (set(GEMM_COVERAGE) | set(UNREACHABLE)) - gemm_symbols
    assert not stale, f"GEMM_COVERAGE / UNREACHABLE name symbols the library does not have: {sorted(stale)}"
    assert not set(GEMM_COVERAGE) & set(UNREACHABLE)


def test_every_covered_kernel_is_what_its_case_launches():
    """the plan of each named case (dvt_gemm_plan at 256 CUs) names the symbol's configuration, layout, epilogue and output"""
    cache = {}
    for sym, case in GEMM_COVERAGE.items():
        if case not in cache:
            cache[case] = _case_symbols(case)
        assert sym in cache[case], f"{case} launches {sorted(cache[case])}, not {sym}"


def test_unreachable_combinations_are_never_planned():
    """the configurations UNREACHABLE names are ones no dvt_gemm call is planned on, over a sweep of shapes, layouts,
    epilogues and outputs"""
    from dvt_amd import ops
    seen = set()
    for dt in (torch.bfloat16, torch.float16):
        for M, N, K in ((4096, 3072, 256), (3000, 2040, 512), (1024, 1024, 8192), (512, 256, 32768), (24576, 512, 512),
                        (8192, 8192, 1024), (256, 256, 2504)):
            for ak in (True, False):
                for bk in (True, False):
                    for epi in range(6):
                        for of in (False, True):
                            if of and epi == 1:
                                continue
                            A = torch.empty(M if ak else K, K if ak else M, dtype=dt)
                            B = torch.empty(N if bk else K, K if bk else N, dtype=dt)
                            kw = dict(a_kmajor=ak, b_kmajor=bk, lda=A.shape[1], ldb=B.shape[1], epilogue=epi,
                                      out_dtype=torch.float32 if of else dt)
                            if epi == 3:
                                kw["residual"] = torch.empty(M, N, dtype=dt)
                            if epi in (1, 4, 5):
                                kw["aux"] = torch.empty(M, N, dtype=dt)
                            p = ops.gemm_plan(A, B, M, N, K, **kw)
                            seen |= symbols_of(p, _T["bf16" if dt == torch.bfloat16 else "fp16"], of)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))
    assert {s for s in seen if s.startswith("gemm_dma_kernel")} <= set(GEMM_COVERAGE)


def test_plan_follows_the_descriptor():
    """a changed epilogue, layout, output type, workspace or carry changes the reported plan"""
    from dvt_amd import ops
    from tests import test_gpu_gemm_exact as G
    kw, ctx = G.build("dma5_tt_none-bf16", "cpu", fill=False)
    base = ops.gemm_plan(ctx["Av"], ctx["Bv"], 4096, 3072, 256, **kw)
    assert base == ops.GemmPlan("dma", 5, 1, 256)
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 4096, 3072, 256, **dict(kw, epilogue=1)).cfg == 3
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 4096, 3072, 256, **dict(kw, out_dtype=torch.float32, out=None)).kernel == "mfma128"
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 4096, 3072, 256, **dict(kw, b_kmajor=False, ldb=3072 + 8)) != base
    kw, ctx = G.build("small_tt32-fp16", "cpu", fill=False)
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 264, 512, 512, **kw).kernel == "small"
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 264, 512, 504, **dict(kw, split_k=2)).kernel == "mfma128"
    assert ops.gemm_plan(ctx["Av"], ctx["Bv"], 264, 512, 500, **kw).kernel == "generic64"             # K % 8, k-major


# ---------------------------------------------------------------- the operands see the faults
@pytest.mark.parametrize("M,N,K", [(64, 64, 128), (64, 64, 200), (512, 32, 4096)])
def test_exact_operands_see_every_missing_kstep(M, N, K):
    """for each builder shape: dropping or doubling any 16- / 32-wide k-step (any chunk-wide one for deep K), swapping two
    k positions of one operand inside a chunk, or shifting a 16 x 16 output fragment changes many outputs"""
    A, B = X.operands(M, N, K, seed=K)
    C = A @ B
    assert torch.equal(C, C.round())
    X.check_bound(C, torch.bfloat16)
    ch = X.chunk_for(K)
    for step in sorted({16, 32, ch}):
        if step < ch:
            continue
        for k0, part in X.kstep_partials(A, B, step):
            changed = int((part != 0).sum())
            assert changed == M * N, f"k-step [{k0}, {k0 + step}) leaves {M * N - changed} outputs unchanged"
            assert not torch.equal(C - part, C) and not torch.equal(C + part, C)
    for c0 in range(0, min(K, 2 * ch), ch):
        for p in range(c0, min(K, c0 + ch) - 1, max(1, ch // 16)):
            d = int((X.swapped_k(A, B, p, p + 1) != C).sum())
            assert d >= 8, f"swapping k positions {p}, {p + 1} changes only {d} outputs"
    for i in range(M // 16 - 1):
        for j in range(N // 16 - 1):
            for di, dj in ((1, 0), (0, 1)):
                d = int((X.shifted_fragment(C, i, j, di, dj) != C).sum())
                assert d >= 128, f"shifting fragment ({i}, {j}) by ({di}, {dj}) changes only {d} of 256 outputs"
