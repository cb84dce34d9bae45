"""CPU gate on the direct tests of the data-movement kernels of csrc/conv.hip: every symbol of the built library whose
kernel name is one of KERNELS -- the im2col / col2im, weight pack / unpack, pad, layout and pixel-pair kernels, i.e. exactly
what the BatchNorm / max-pool gate (tests/test_batchnorm_coverage.py) leaves out of its scope -- is tied to a named
parameter set of tests/test_gpu_conv_data.py, and the symbol's template arguments (element types, NCHW) are derived from
that set's parameters through the dispatch mirrors of tests/convdata_ref.py: a row that names a case of another dtype or
another route fails.  ``transpose_kernel`` stays with tests/test_rowwise_coverage.py, which already has its cases.  Only the
names of the listing are read."""
import importlib
import os
import re
import sys

import pytest

from tests import convdata_ref as V
from tests import test_batchnorm_coverage as BN
from tests import test_rowwise_coverage as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE = "tests.test_gpu_conv_data"

ELSEWHERE = {"transpose_kernel"}                      # tests/test_rowwise_coverage.py
KERNELS = ["im2col_kernel", "im2col_nchw_stem_kernel", "im2col_nhwc_vec_kernel", "col2im_nhwc_kernel", "col2im_scalar_kernel",
           "weight_pack_kernel", "weight_unpack_kernel", "weight_unpack_t_kernel", "weight_pack_dgrad_kernel",
           "weight_pack_group_kernel", "pad3_kernel", "unpad3_kernel", "nchw_to_nhwc_pad8_kernel", "nchw_to_nhwc_pair4_kernel",
           "conv_weight_pairs_kernel", "conv_weight_pairs_bwd_kernel"]
# symbols of KERNELS that no entry point can launch, each with its reason (none: every instantiation has a dispatch branch)
UNREACHABLE = {}
SYMBOL_FLOOR = 62

# kernels without template arguments: the test function that calls their entry point, and the case named for them
PLAIN = {"weight_unpack_kernel": ("test_weight_unpack", "test_weight_unpack[True]"),
         "weight_unpack_t_kernel": ("test_weight_unpack_t", "test_weight_unpack_t[True]"),
         "pad3_kernel": ("test_pad3", "test_pad3[3x5x6-to-4x8x6]"),
         "unpad3_kernel": ("test_unpad3", "test_unpad3[True]"),
         "conv_weight_pairs_kernel": ("test_weight_pairs", "test_weight_pairs[3-kw7pw3kwp4]"),
         "conv_weight_pairs_bwd_kernel": ("test_weight_pairs_bwd", "test_weight_pairs_bwd[True-3-kw7pw3kwp4]"),
         "weight_pack_group_kernel": ("test_pack_group", "test_pack_group[bf16-elems-rowlen]")}


def _table():
    cov = {}
    b = lambda v: "true" if v else "false"
    for s, d in V.PAIRS7:
        S, D = V.CXX[s], V.CXX[d]
        for nchw in (False, True):
            cov[f"im2col_kernel<{S}, {D}, {b(nchw)}>"] = f"test_im2col[{s}-{d}-{'nchw' if nchw else 'nhwc'}]"
        cov[f"im2col_nchw_stem_kernel<{S}, {D}, 3, 7, 7>"] = f"test_im2col_stem[{s}-{d}]"
        cov[f"col2im_scalar_kernel<{S}, {D}, true>"] = f"test_col2im_nchw[{s}-{d}]"
    for n, t in V.CXX.items():
        cov[f"im2col_nhwc_vec_kernel<{t}>"] = f"test_im2col_vec[{n}-16]"
        cov[f"col2im_nhwc_kernel<{t}>"] = f"test_col2im_nhwc[{n}-c16-add-compact]"
        cov[f"col2im_scalar_kernel<{t}, {t}, false>"] = f"test_col2im_scalar[{n}-kw7-sw1]"
        cov[f"weight_pack_kernel<{t}>"] = f"test_weight_pack[{n}-6]"
        cov[f"weight_pack_dgrad_kernel<{t}>"] = f"test_weight_pack_dgrad[{n}]"
    for s, d in V.PAIRS6:
        cov[f"nchw_to_nhwc_pad8_kernel<{V.CXX[s]}, {V.CXX[d]}>"] = f"test_nhwc_pad8[{s}-{d}-3]"
        cov[f"nchw_to_nhwc_pair4_kernel<{V.CXX[s]}, {V.CXX[d]}>"] = f"test_nhwc_pair4[{s}-{d}-3]"
    for k, (_, case) in PLAIN.items():
        cov[k] = case
    return cov


COVERAGE = _table()


def test_the_two_gates_partition_conv_hip():
    """KERNELS is exactly what the BatchNorm / max-pool gate leaves out, less the transpose, which the row-kernel gate holds"""
    assert set(KERNELS) | ELSEWHERE == BN.OUT_OF_SCOPE and not set(KERNELS) & ELSEWHERE and len(set(KERNELS)) == len(KERNELS)
    assert BN._defined() == set(BN.KERNELS) | set(KERNELS) | ELSEWHERE
    assert {k.split("<")[0] for k in COVERAGE} | {k.split("<")[0] for k in UNREACHABLE} == set(KERNELS)
    for t in V.CXX.values():
        assert RW.COVERAGE[("conv.hip", f"transpose_kernel<{t}>")].startswith("test_gpu_rowwise::test_transpose_last2[")
    assert "transpose_kernel" in RW.SCOPE["conv.hip"]


@pytest.fixture(scope="module")
def symbols():
    """the listing's kernels whose name is one of KERNELS, without their argument lists"""
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from isa_listing import kernel_listings
    finally:
        sys.path.pop(0)
    out = set()
    for s in kernel_listings(dvt_amd._lib.LIB_PATH, demangle=True):
        short = BN._short(s)
        m = re.match(r"\w+", short)
        if m and m.group(0) in KERNELS:
            out.add(short)
    return out


def _missing_and_stale(symbols, table, unreachable=UNREACHABLE):
    placed = set(table) | set(unreachable)
    return symbols - placed, placed - symbols


def test_every_data_movement_kernel_has_a_direct_gpu_case(symbols):
    per_kernel = {}
    for s in symbols:
        k = re.match(r"\w+", s).group(0)
        per_kernel[k] = per_kernel.get(k, 0) + 1
    print(f"data-movement kernel symbols in the listing ({len(symbols)}): {sorted(per_kernel.items())}")
    assert len(symbols) >= SYMBOL_FLOOR, "the listing has fewer of these kernels than it had: the disassembly found too little"
    assert set(per_kernel) == set(KERNELS), f"kernels without any symbol: {sorted(set(KERNELS) - set(per_kernel))}"
    missing, stale = _missing_and_stale(symbols, COVERAGE)
    assert not missing, f"kernels without a direct GPU case in COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE / UNREACHABLE name kernels the library does not have: {sorted(stale)}"
    assert not set(COVERAGE) & set(UNREACHABLE) and all(isinstance(r, str) and r for r in UNREACHABLE.values())


def _case_params(case):
    """(function name, parameter set) of a named case of tests/test_gpu_conv_data.py; asserts that the case exists"""
    fn_name, ident = re.match(r"^(\w+)\[(.+)\]$", case).groups()
    module = importlib.import_module(GPU_FILE)
    assert hasattr(module, fn_name), case
    sets = dict(BN._param_sets(getattr(module, fn_name)))
    assert ident in sets, f"{case}: no such parameter set (has {sorted(sets)[:8]} ...)"
    return fn_name, sets[ident]


def _launched(fn, p):
    """the symbols of KERNELS the case ``fn[p]`` launches, by the dispatch mirrors"""
    T = importlib.import_module(GPU_FILE)
    K = T._K
    if fn == "test_im2col":
        return {V.im2col_route(p["pair"][0], p["pair"][1], p["layout"] == "nchw", C, k, K(C, k) + extra, True)
                for C, H, W, k, s, pd, extra in T.IM2COL_GEOMS}
    if fn == "test_im2col_fallbacks":
        src, dst, nchw, C, H, W, k, s, pd, extra, mis = T.IM2COL_FALLBACKS[p["case"]]
        return {V.im2col_route(src, dst, nchw, C, k, K(C, k) + extra, not mis)}
    if fn == "test_im2col_stem":
        return {V.im2col_route(p["pair"][0], p["pair"][1], True, 3, 7, ld, True) for H, W, s, pd, ld in T.STEM_GEOMS}
    if fn == "test_im2col_vec":
        return {V.im2col_route(p["name"], p["name"], False, p["C"], T.VEC_GEOM[2], K(p["C"], T.VEC_GEOM[2]), True)}
    if fn == "test_col2im_nhwc":
        C, H, W, k, s, pd, extra, add = T.C2I_VEC[p["case"]]
        return {V.col2im_route(p["name"], C, K(C, k) + extra, True, add is not None)}
    if fn == "test_col2im_scalar":
        C, H, W, k, s, pd, extra, mis = T.C2I_SCALAR[p["case"]]
        return {V.col2im_route(p["name"], C, K(C, k) + extra, not mis)}
    if fn == "test_col2im_nchw":
        return {V.col2im_nchw_route(*p["pair"])}
    if fn == "test_weight_pack":
        return {f"weight_pack_kernel<{V.CXX[p['name']]}>"}
    if fn == "test_weight_pack_dgrad":
        return {f"weight_pack_dgrad_kernel<{V.CXX[p['name']]}>"}
    if fn == "test_nhwc_pad8":
        return {V.nhwc_pad_route(p["pair"][0], p["pair"][1], 8)}
    if fn == "test_nhwc_pair4":
        return {V.nhwc_pad_route(p["pair"][0], p["pair"][1], 4)}
    plain = {f: k for k, (f, _) in PLAIN.items()}
    assert fn in plain, f"{fn} is not a case of a kernel of this gate"
    return {plain[fn]}


def _check_row(sym, case):
    """the named set exists and what it runs is the symbol's instantiation, and nothing else of this family"""
    fn, p = _case_params(case)
    assert _launched(fn, p) == {sym}, f"{case} does not run {sym} (it runs {sorted(_launched(fn, p))})"


def test_every_named_case_exists_and_runs_the_symbols_instantiation():
    for sym, case in COVERAGE.items():
        _check_row(sym, case)


def test_the_gate_fails_when_a_row_is_deleted_stale_or_mismatched(symbols):
    """the properties the gate exists for, on copies of the table"""
    for key in COVERAGE:                                  # deleting any one row
        table = dict(COVERAGE)
        del table[key]
        missing, stale = _missing_and_stale(symbols, table)
        assert missing == {key} and not stale
        assert _missing_and_stale(symbols, table, {key: "a reason"}) == (set(), set())
    table = dict(COVERAGE)
    table["im2col_nchw_stem_kernel<float, float, 3, 3, 3>"] = "test_im2col_stem[fp32-fp32]"       # no such instantiation
    assert _missing_and_stale(symbols, table) == (set(), {"im2col_nchw_stem_kernel<float, float, 3, 3, 3>"})
    assert _missing_and_stale(symbols, COVERAGE, {"col2im_scalar_kernel<float, _Float16, false>": "never instantiated"})[1]
    for sym, case in (("im2col_kernel<float, float, false>", "test_im2col[fp32-bf16-nhwc]"),           # another destination type
                      ("im2col_kernel<float, float, false>", "test_im2col[fp32-fp32-nchw]"),           # the other layout
                      ("im2col_kernel<float, float, false>", "test_im2col[fp32-fp32-nwhc]"),           # no such set
                      ("im2col_kernel<float, float, true>", "test_im2col_stem[fp32-fp32]"),            # the stem kernel takes it
                      ("im2col_nchw_stem_kernel<float, float, 3, 7, 7>", "test_im2col_fallbacks[nchw3k7-ld147]"),
                      ("im2col_nhwc_vec_kernel<std::bfloat16_t>", "test_im2col_fallbacks[nhwc8-misaligned]"),
                      ("im2col_nhwc_vec_kernel<float>", "test_im2col_vec[bf16-8]"),
                      ("im2col_nhwc_vec_kernel<float>", "test_im2col[fp32-fp32-nhwc]"),                # C = 5: the general kernel
                      ("col2im_nhwc_kernel<float>", "test_col2im_scalar[fp32-c8-misaligned]"),
                      ("col2im_scalar_kernel<float, float, false>", "test_col2im_nhwc[fp32-c8-k3s2p1]"),
                      ("col2im_scalar_kernel<float, float, false>", "test_col2im_nchw[fp32-fp32]"),    # NCHW = true
                      ("col2im_scalar_kernel<float, _Float16, true>", "test_col2im_nchw[fp16-fp32]"),  # the pair the other way round
                      ("weight_pack_kernel<float>", "test_weight_pack_dgrad[fp32]"),
                      ("weight_pack_kernel<float>", "test_weight_pack[bf16-0]"),
                      ("nchw_to_nhwc_pad8_kernel<float, _Float16>", "test_nhwc_pair4[fp32-fp16-3]"),
                      ("nchw_to_nhwc_pair4_kernel<float, _Float16>", "test_nhwc_pair4[fp32-bf16-3]"),
                      ("unpad3_kernel", "test_pad3[identity]"),
                      ("conv_weight_pairs_kernel", "test_weight_pairs_bwd[True-3-kw7pw3kwp4]"),
                      ("weight_pack_group_kernel", "test_weight_pack[fp32-0]")):
        with pytest.raises(AssertionError):
            _check_row(sym, case)
