"""CPU gate on the convolution family's exact tests: every gemm_dma_kernel<..., true> (implicit-GEMM convolution),
conv_split_reduce_kernel and splitk_reduce_conv_tiled_kernel symbol of the built library is either launched by a named
case of tests/test_gpu_conv_exact.py -- the library's own plan query (dvt_conv2d_implicit_plan, at 256 CUs) says that case
takes that instantiation -- or listed as unreachable with a reason, which a plan sweep confirms; the convolution-scatter
mode of splitk_reduce_pending_kernel (a run-time mode: no symbol of its own) has a named case whose plan reports it; and
the operands of those cases see a missing, doubled or misplaced tap, channel range, pixel, slice, k-tile, row or fragment."""
import re

import pytest
import torch

from tests import conv_exact as V
from tests import gemm_exact as X
from tests import test_gpu_conv_exact as G
from tests.test_gemm_coverage import _short

_T = {"bf16": "std::bfloat16_t", "fp16": "_Float16"}

# configuration -> the forward case that launches it (its `stats` run: epilogue NONE, its `res` run: RESIDUAL)
FWD_OF_CFG = {0: "f0_n144", 1: "f1_c32", 4: "f4_stem", 6: "f6_c64", 7: "f7_13", 9: "f9_n512", 10: "f10_n128"}
SPLIT_OF_CFG = {9: "s9_uneven", 10: "s10_ragged"}                  # slab kernels; both launch conv_split_reduce_kernel
WGRAD_OF_CFG = {0: "w0_split3", 1: "w1_n288", 6: "w6_ragged", 7: "w7_split4"}
TILED_CASE = "w0_tiled"                                            # splitk_reduce_conv_tiled_kernel
SCATTER_CASE = "w7_padded"                                         # splitk_reduce_pending_kernel, conv_taps != 0

# every kernel symbol of the family -> the exact GPU case that launches it
CONV_COVERAGE = {}
for _d, _e in _T.items():
    for _cfg, _n in FWD_OF_CFG.items():
        CONV_COVERAGE[f"gemm_dma_kernel<{_e}, true, true, {_cfg}, 0, 0, true>"] = f"test_conv_forward_exact[{_n}-stats-{_d}]"
        CONV_COVERAGE[f"gemm_dma_kernel<{_e}, true, true, {_cfg}, 3, 0, true>"] = f"test_conv_forward_exact[{_n}-res-{_d}]"
    for _cfg, _n in SPLIT_OF_CFG.items():
        CONV_COVERAGE[f"gemm_dma_kernel<{_e}, true, true, {_cfg}, 0, 2, true>"] = f"test_conv_forward_exact[{_n}-stats-{_d}]"
    for _cfg, _n in WGRAD_OF_CFG.items():
        CONV_COVERAGE[f"gemm_dma_kernel<{_e}, false, false, {_cfg}, 0, 2, true>"] = f"test_conv_wgrad_exact[{_n}-{_d}]"
    CONV_COVERAGE[f"conv_split_reduce_kernel<{_e}>"] = f"test_conv_forward_exact[s9_uneven-res-{_d}]"
CONV_COVERAGE["splitk_reduce_conv_tiled_kernel"] = f"test_conv_wgrad_exact[{TILED_CASE}-bf16]"

UNREACHABLE = {
    f"gemm_dma_kernel<{_e}, false, false, 4, 0, 2, true>":
        "conv_cfg puts every weight gradient of at most 64 output channels on configuration 6 (its k-tile runs over pixels: "
        "any C % 8 == 0 takes the 64-deep form), so conv_wgrad_plan never picks configuration 4"
    for _e in _T.values()}

_FAMILY = re.compile(r"^(gemm_dma_kernel<.*, true>|conv_split_reduce_kernel<.*>|splitk_reduce_conv_tiled_kernel)$")


@pytest.fixture(scope="module")
def conv_symbols():
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


def symbols_of(plan, e, wgrad):
    """the kernel symbols of the family a call with this plan launches (e: element type)"""
    o = {"map": 0, "slab": 2}[plan.out]
    ab = "false, false" if wgrad else "true, true"
    out = {f"gemm_dma_kernel<{e}, {ab}, {plan.cfg}, {plan.epilogue}, {o}, true>"}
    if plan.reduce == "split":
        out.add(f"conv_split_reduce_kernel<{e}>")
    if not plan.deferred and "scatter_tiled" in (plan.reduce, plan.carry_reduce):
        out.add("splitk_reduce_conv_tiled_kernel")
    if plan.deferred and plan.carry_reduce == "scatter_tiled":
        out.add("splitk_reduce_conv_tiled_kernel")
    return out


def _case_symbols(case):
    """the symbols a named GPU case launches, from the library's plan query at 256 CUs (no device)"""
    fn, params = re.match(r"^(\w+)\[(.+)\]$", case).groups()
    assert hasattr(G, fn), case
    if fn == "test_conv_forward_exact":
        name, how, dname = params.rsplit("-", 2)
        assert name in G.FWD_CASES and how in ("stats", "res") and dname in G.DTYPES, case
        res = how == "res"
        plan = G.fwd_plan(name, G.DTYPES[dname], residual=res, want_stats=not res)
        assert plan == G.expected_fwd_plan(name, res), case
        return symbols_of(plan, _T[dname], False)
    if fn == "test_conv_wgrad_exact":
        name, dname = params.rsplit("-", 1)
        assert name in G.WGRAD_CASES and dname in G.DTYPES, case
        c = G.WGRAD_CASES[name]
        packed = G.wgrad_plan(name, G.DTYPES[dname])
        master = G.wgrad_plan(name, G.DTYPES[dname], master=True, accumulate=True, logical=c["logical"])
        assert packed == G.expected_wgrad_plan(name, False, False) and master == G.expected_wgrad_plan(name, True, False), case
        return symbols_of(packed, _T[dname], True) | symbols_of(master, _T[dname], True)
    raise AssertionError(f"unknown case {case}")


def test_every_conv_kernel_has_an_exact_gpu_case(conv_symbols):
    assert len(conv_symbols) > 40, "the listing has (almost) no convolution kernels: the disassembly found nothing"
    missing = conv_symbols - set(CONV_COVERAGE) - set(UNREACHABLE)
    assert not missing, f"convolution kernels without an exact GPU case in CONV_COVERAGE (or a reason in UNREACHABLE): {sorted(missing)}"
    stale = (set(CONV_COVERAGE) | set(UNREACHABLE)) - conv_symbols
    assert not stale, f"CONV_COVERAGE / UNREACHABLE name symbols the library does not have: {sorted(stale)}"
    assert not set(CONV_COVERAGE) & set(UNREACHABLE)


def test_every_covered_kernel_is_what_its_case_launches():
    cache = {}
    for sym, case in CONV_COVERAGE.items():
        if case not in cache:
            cache[case] = _case_symbols(case)
        assert sym in cache[case], f"{case} launches {sorted(cache[case])}, not {sym}"


def test_every_case_states_the_plan_the_library_reports():
    """every named case, covered symbol or not: the plan it asserts on the GPU is the plan at 256 CUs (so a case whose
    expectation is wrong fails here, without a GPU)"""
    from dvt_amd import ops
    for dt in G.DTYPES.values():
        for name in G.FWD_CASES:
            for res in (False, True):
                assert G.fwd_plan(name, dt, residual=res, want_stats=not res) == G.expected_fwd_plan(name, res), name
        for name, c in G.WGRAD_CASES.items():
            assert G.wgrad_plan(name, dt) == G.expected_wgrad_plan(name, False, False), name
            for defer in (False, True):
                p = G.wgrad_plan(name, dt, master=True, accumulate=True, logical=c["logical"], defer_reduce=defer)
                assert p == G.expected_wgrad_plan(name, True, defer), name
        for name, c in G.DGRAD_CASES.items():
            Cout = c["geom"][4]
            for cls in G.dgrad_classes(name):
                for res in (False, True):
                    want = ops.ConvPlan(c["cfg"], 1, cls[2][0] * cls[2][1] * Cout, G.RES if res else G.NONE)
                    assert G.dgrad_class_plan(name, cls, dt, res, False) == want, (name, cls)


def test_the_scatter_mode_of_the_pending_reduce_has_a_named_case():
    """splitk_reduce_pending_kernel with conv_taps != 0 is one symbol with the plain GEMM reduce: its named case
    (test_conv_wgrad_exact[w7_padded-*], master layout, channel-padded, accumulate) is planned on the plain scatter, alone
    and deferred; the tiled case on the tiled one; and every other weight-gradient case names one of the two"""
    for dname, dt in G.DTYPES.items():
        c = G.WGRAD_CASES[SCATTER_CASE]
        for defer in (False, True):
            p = G.wgrad_plan(SCATTER_CASE, dt, master=True, accumulate=True, logical=c["logical"], defer_reduce=defer)
            assert p.reduce == "scatter" and p.deferred == defer
        assert G.wgrad_plan(TILED_CASE, dt, master=True).reduce == "scatter_tiled"
        for name, w in G.WGRAD_CASES.items():
            assert G.wgrad_plan(name, dt, master=True, logical=w["logical"]).reduce == w["scatter"], name


def _sweep():
    for dname, dt in G.DTYPES.items():
        for N, H, W in ((1, 7, 7), (3, 14, 14), (8, 28, 28), (16, 56, 56), (64, 56, 56)):
            for Cc in (8, 24, 32, 64, 96, 144, 256, 1152):
                for Cout in (8, 64, 72, 128, 144, 256, 288, 512, 1152):
                    for k, stride, pad in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), ((3, 1), 1, (1, 0)), ((1, 3), (1, 2), (0, 1)),
                                           (7, 2, 3)):
                        yield dname, dt, (N, Cc, H, W, Cout, k, stride, pad)


def test_unreachable_instantiations_are_never_planned():
    """over a sweep of shapes, strides, channel counts and both dtypes no descriptor is planned on an UNREACHABLE symbol, and
    every symbol that is planned has a case"""
    from dvt_amd import ops
    seen = set()
    for dname, dt, g in _sweep():
        for res in (False, True):
            seen |= symbols_of(ops.conv2d_implicit_plan(*g, dt, residual=res), _T[dname], False)
        seen |= symbols_of(ops.conv2d_implicit_plan(*g, dt, wgrad=True, master=True), _T[dname], True)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))
    assert seen <= set(CONV_COVERAGE), sorted(seen - set(CONV_COVERAGE))
    assert len(seen) >= len(CONV_COVERAGE) - 2          # (the sweep itself reaches the family, all but at most two symbols)


def test_plan_follows_the_descriptor():
    """a changed residual, split workspace, carry or dtype changes the reported plan"""
    from dvt_amd import ops, _lib as L
    base = G.fwd_plan("f10_n128", G.BF)
    assert base == ops.ConvPlan(10, 1, 576) == G.fwd_plan("f10_n128", G.FP)       # (the dtype picks the symbol, not the plan)
    assert symbols_of(base, _T["bf16"], False) != symbols_of(G.fwd_plan("f10_n128", G.FP), _T["fp16"], False)
    assert G.fwd_plan("f10_n128", G.BF, residual=True).epilogue == G.RES
    with pytest.raises(RuntimeError, match="exclusive"):
        G.fwd_plan("f10_n128", G.BF, residual=True, want_stats=True)
    with pytest.raises(RuntimeError, match="16-bit"):
        G.fwd_plan("f10_n128", torch.float32)
    pend = L.SplitKPending(valid=1, splits=2, M=576, N=128, conv_taps=9, conv_cin=64)
    assert G.fwd_plan("f10_n128", G.BF, carry=pend)[-2:] == ("tail", "none")
    assert G.fwd_plan("s10_ragged", G.BF, carry=pend)[-2:] == ("alone", "scatter")
    big = L.SplitKPending(valid=1, splits=2, M=2376, N=520, conv_taps=9, conv_cin=264)
    assert G.fwd_plan("s10_ragged", G.BF, carry=big)[-2:] == ("alone", "scatter_tiled")
    assert G.fwd_plan("s10_ragged", G.BF, carry=L.SplitKPending(valid=1, splits=2, M=576, N=128))[-2:] == ("alone", "plain")
    assert G.fwd_plan("s10_ragged", G.BF, carry=L.SplitKPending(valid=0))[-2:] == ("none", "none")
    split = G.fwd_plan("s10_ragged", G.BF, residual=True)
    assert (split.out, split.reduce, split.epilogue) == ("slab", "split", G.NONE)   # the reduce adds the residual
    with pytest.raises(RuntimeError, match="workspace"):                             # a split launch has no unsplit fallback
        G.fwd_plan("s10_ragged", G.BF, workspace=False)
    with pytest.raises(RuntimeError, match="workspace"):
        G.wgrad_plan("w7_split4", G.BF, workspace=False)
    # scattered class launches stay unsplit whatever their depth
    c = G.FWD_CASES["s10_ragged"]
    assert ops.conv2d_implicit_plan(c["N"], c["C"], c["H"], c["W"], c["Cout"], c["k"], 1, 1, G.BF, out_hw=(7, 7), out_rows=True).split == 1
    w = G.wgrad_plan("w7_split4", G.BF)
    assert (w.reduce, w.deferred) == ("plain", False)
    assert G.wgrad_plan("w7_split4", G.BF, defer_reduce=True) == w._replace(deferred=True)
    assert G.wgrad_plan("w7_split4", G.BF, master=True).reduce == "scatter"


# ---------------------------------------------------------------- bounds on the CPU
@pytest.mark.parametrize("name", list(G.FWD_CASES))
def test_forward_references_are_exact_in_both_types(name):
    b = G.build_fwd(name)
    for dt in G.DTYPES.values():
        X.check_bound(b["y"], dt)
        X.check_bound(b["y"] + b["res"], dt)
    assert torch.equal(b["y"], b["y"].round())
    V.check_stats_bound(b["y"], G.stats_rows(name))


@pytest.mark.parametrize("name", list(G.DGRAD_CASES))
def test_dgrad_references_are_exact_in_both_types(name):
    b = G.build_dgrad(name)
    for dt in G.DTYPES.values():
        X.check_bound(b["want"], dt)
        X.check_bound(b["dx"], dt)


@pytest.mark.parametrize("name", list(G.WGRAD_CASES))
def test_wgrad_references_are_exact_in_fp32(name):
    b = G.build_wgrad(name)
    assert torch.equal(b["dW"], b["dW"].round()) and float(b["dW"].abs().max()) + 4 < 2 ** 24
    # every partial sum too: the sum of the magnitudes is an exact fp32 integer
    assert float(V.wgrad_ref(b["x"], b["dz"].abs(), G.WGRAD_CASES[name]["k"], G.WGRAD_CASES[name]["stride"],
                             G.WGRAD_CASES[name]["pad"]).max()) < 2 ** 24


# ---------------------------------------------------------------- the operands see the faults
@pytest.mark.parametrize("name", list(G.FWD_CASES))
def test_forward_operands_see_the_faults(name):
    """dropping or doubling any (tap, 16-channel range) changes every output whose tap is in bounds and none of the others
    (so one tap dropped at one border pixel shows in that pixel's row); a gather one pixel off in h or w, a dropped split
    slice and a shifted 16 x 16 output fragment change the reference in most of the elements they touch"""
    c, b = G.FWD_CASES[name], G.build_fwd(name)
    x, w, y = b["x"], b["w"], b["y"]
    kh, kw = V.pair(c["k"])
    Cout = c["Cout"]
    tap_total = {}
    for ki in range(kh):
        for kj in range(kw):
            for lo, hi in V.channel_ranges(c["C"]):
                part, inb = V.tap_range_partial(x, w, c["stride"], c["pad"], ki, kj, lo, hi, c["trim_w"])
                assert bool((part[inb] != 0).all()), f"tap ({ki}, {kj}) channels [{lo}, {hi}) adds nothing to some in-bounds output"
                assert bool((part[~inb] == 0).all()), f"tap ({ki}, {kj}) adds to an output it is padded at"
                tap_total[(ki, kj)] = tap_total.get((ki, kj), 0) + part
    # one tap dropped at one border pixel: that pixel's row changes in every column whose tap sum is nonzero -- at the
    # pixels where some tap IS padded (the border), for each tap that is not: most of the Cout elements a fault touches
    some_padded = torch.zeros(y.shape[0], dtype=torch.bool)
    inbs = {}
    for (ki, kj) in tap_total:
        inbs[(ki, kj)] = V.tap_range_partial(x, w, c["stride"], c["pad"], ki, kj, 0, 1, c["trim_w"])[1]
        some_padded |= ~inbs[(ki, kj)]
    for t, tot in tap_total.items():
        rows = some_padded & inbs[t]
        if bool(rows.any()):
            changed = (tot[rows] != 0).sum(1)
            assert int(changed.min()) >= Cout // 2, f"dropping tap {t} at a border pixel changes only {int(changed.min())} of {Cout} columns"
    if kh * kw > 1:
        assert bool(some_padded.any()) or V.pair(c["pad"]) == (0, 0)
    # the gathered pixel one off
    for dh, dw in ((1, 0), (0, 1)):
        off = V.conv_ref(V.shifted_map(x, dh, dw), w, c["stride"], c["pad"], c["trim_w"])
        assert bool((off != y).any(1).all()), f"a gather shifted by ({dh}, {dw}) leaves some output rows unchanged"
        assert int((off != y).sum()) * 2 >= y.numel()
    # a dropped slice of the split reduction
    if c["split"] > 1:
        col, wp = V.im2col(x, c["k"], c["stride"], c["pad"], c["trim_w"]), b["wp"]
        for z in range(c["split"]):
            k0, k1 = z * c["kps"], min(col.shape[1], (z + 1) * c["kps"])
            assert k0 < k1
            part = col[:, k0:k1] @ wp[:, k0:k1].t()
            assert int((part != 0).sum()) * 2 >= y.numel(), f"dropping slice {z} changes under half of the outputs"
    # a 16 x 16 output fragment taken from its neighbour
    for i in sorted({0, y.shape[0] // 32, y.shape[0] // 16 - 2}):
        for j in range(Cout // 16 - 1):
            for di, dj in ((1, 0), (0, 1)):
                dchg = int((X.shifted_fragment(y, i, j, di, dj) != y).sum())
                assert dchg >= 128, f"shifting fragment ({i}, {j}) by ({di}, {dj}) changes only {dchg} of 256 outputs"


@pytest.mark.parametrize("name", list(G.WGRAD_CASES))
def test_wgrad_operands_see_every_pixel_tile(name):
    """dropping any k-tile of pixels -- the ragged last one too -- or a whole slice, or shifting a 16 x 16 fragment of dWt,
    changes most of the entries it touches"""
    c, b = G.WGRAD_CASES[name], G.build_wgrad(name)
    Cout = c["Cout"]
    col = V.im2col(b["x"], c["k"], c["stride"], c["pad"], c["trim_w"])
    dz = b["dz"].reshape(-1, Cout)
    rows, tk = dz.shape[0], (32 if c["cfg"] in (1, 4) else 64)
    full = col.t() @ dz
    kh, kw = V.pair(c["k"])
    assert torch.equal(full, b["dW"].permute(2, 3, 1, 0).reshape(kh * kw * c["C"], Cout))
    steps = sorted({(r0, min(rows, r0 + tk)) for r0 in range(0, rows, tk)} | {(z * c["kps"], min(rows, (z + 1) * c["kps"])) for z in range(c["split"])})
    for r0, r1 in steps:
        part = col[r0:r1].t() @ dz[r0:r1]
        assert int((part != 0).sum()) * 2 >= part.numel(), f"dropping pixels [{r0}, {r1}) changes under half of dWt"
    assert (rows % tk != 0) == (name in ("w6_ragged", "w7_31_s2", "w0_split3", "w1_n288", "w0_tiled"))
    for i in (0, full.shape[0] // 16 - 2):
        for j in range(0, Cout // 16 - 1, 3):
            for di, dj in ((1, 0), (0, 1)):
                assert int((X.shifted_fragment(full, i, j, di, dj) != full).sum()) >= 128


@pytest.mark.parametrize("name", list(G.DGRAD_CASES))
def test_dgrad_operands_see_a_misplaced_row(name):
    """moving one out_rows entry to a neighbouring pixel: neighbouring rows of the result differ (in most channels), with and
    without the shortcut's gradient; and the classes' rows written out here are the library's table"""
    from dvt_amd import ops
    b = G.build_dgrad(name)
    N, Cin, H, Wd, Cout, k, stride, pad = G.DGRAD_CASES[name]["geom"]
    sh, sw = V.pair(stride)
    for ref in (b["dx"], b["want"]):
        for step in (1, Wd):
            diff = (ref[step:] != ref[:-step]).sum(1)
            assert int(diff.min()) >= Cin // 2, f"rows {step} apart share all but {int(diff.min())} of {Cin} channels"
    for (a_, b_, *_r) in G.dgrad_classes(name):
        assert torch.equal(G.class_rows(N, H, Wd, sh, sw, a_, b_).to(torch.int32),
                           ops.strided_class_rows(N, H, Wd, sh, sw, a_, b_, "cpu"))
