"""CPU gate on the direct tests of the BatchNorm and max-pool kernels of csrc/conv.hip: every symbol of the built library
whose kernel name is one of KERNELS is tied to a named parameter set of tests/test_gpu_batchnorm.py, and the symbol's
template arguments (element type, MODE, POOL, MSRC, RES, MASK, DRES, CL) are derived from that set's parameters through the
mirrors of tests/batchnorm_ref.py -- a row that names the wrong case fails.  Only the names of the listing are read.

Scope: the statistics, finalize, fold, apply, pooled and max-pool kernels.  conv.hip's other kernels (OUT_OF_SCOPE: the
im2col / col2im, weight pack, pad, layout and pixel-pair kernels) have their own gate, tests/test_conv_data_coverage.py,
over the exact cases of tests/test_gpu_conv_data.py, and the transpose kernel its rows in tests/test_rowwise_coverage.py;
a kernel added to conv.hip later has to be placed in one list or the other."""
import importlib
import itertools
import os
import re
import sys

import pytest

from tests import batchnorm_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ["bn_colstats_kernel", "bn_colstats_scalar_kernel", "bn_colstats_pool_quad_kernel", "bn_finalize_kernel",
           "bn_partial_fold_kernel", "rsqrt_eps_kernel", "bn_apply_fwd_kernel", "bn_apply_fwd_scalar_kernel",
           "bn_apply_bwd_kernel", "bn_apply_bwd_scalar_kernel", "bn_apply_bwd_pool_kernel", "bn_apply_bwd_pool_quad_kernel",
           "maxpool_fwd_kernel", "maxpool_fwd_vec_kernel", "maxpool_bwd_kernel", "maxpool_bwd_vec_kernel",
           "maxpool_bwd_k3s2p1_kernel", "bn_relu_maxpool_k3s2p1_kernel"]
OUT_OF_SCOPE = {"im2col_kernel", "im2col_nchw_stem_kernel", "im2col_nhwc_vec_kernel", "col2im_nhwc_kernel", "col2im_scalar_kernel",
                "weight_pack_kernel", "weight_unpack_kernel", "weight_unpack_t_kernel", "weight_pack_dgrad_kernel",
                "weight_pack_group_kernel", "pad3_kernel", "unpad3_kernel", "nchw_to_nhwc_pad8_kernel",
                "nchw_to_nhwc_pair4_kernel", "conv_weight_pairs_kernel", "conv_weight_pairs_bwd_kernel", "transpose_kernel"}
# symbols of KERNELS that no entry point can launch, each with its reason (none: every instantiation has a dispatch branch)
UNREACHABLE = {}

_T = {"fp32": "float", "bf16": "std::bfloat16_t", "fp16": "_Float16"}
_MSRC = {"z": 0, "y": 1, "mask": 2}
_b = lambda v: "true" if v else "false"


def _table():
    cov = {}
    for n, t in _T.items():
        cov[f"bn_colstats_kernel<{t}, 0, false, 0>"] = f"test_bn_stats[{n}-144]"
        for src, msrc in _MSRC.items():
            cov[f"bn_colstats_kernel<{t}, 1, false, {msrc}>"] = f"test_bn_bwd[{n}-{src}-nodres]"
            for dres in (False, True):
                cov[f"bn_apply_bwd_kernel<{t}, {msrc}, {_b(dres)}>"] = f"test_bn_bwd[{n}-{src}-{'dres' if dres else 'nodres'}]"
        for res, mask in itertools.product((False, True), repeat=2):
            cov[f"bn_apply_fwd_kernel<{t}, {_b(res)}, {_b(mask)}>"] = f"test_bn_apply_fwd[{n}-{res}-{mask}]"
        cov[f"bn_colstats_kernel<{t}, 1, true, 0>"] = f"test_stem_bwd[{n}-16-9x11]"          # odd H and W
        cov[f"bn_apply_bwd_pool_kernel<{t}>"] = f"test_stem_bwd[{n}-64-9x11]"
        cov[f"bn_colstats_pool_quad_kernel<{t}>"] = f"test_stem_bwd[{n}-64-12x16]"           # even H and W
        cov[f"bn_apply_bwd_pool_quad_kernel<{t}>"] = f"test_stem_bwd[{n}-16-2x2]"
        cov[f"bn_relu_maxpool_k3s2p1_kernel<{t}>"] = f"test_stem_fwd[{n}-64-12x16]"
        for k in ("bn_colstats_scalar_kernel<%s, 0>", "bn_colstats_scalar_kernel<%s, 1>", "bn_apply_fwd_scalar_kernel<%s>",
                  "bn_apply_bwd_scalar_kernel<%s>"):
            cov[k % t] = f"test_bn_scalar[{n}-45]"
        cov[f"maxpool_fwd_kernel<{t}>"] = f"test_maxpool_scalar[{n}-45]"
        cov[f"maxpool_bwd_kernel<{t}>"] = f"test_maxpool_scalar[{n}-257]"
        cov[f"maxpool_fwd_vec_kernel<{t}>"] = f"test_maxpool[{n}-k5s2p2]"
        cov[f"maxpool_bwd_vec_kernel<{t}>"] = f"test_maxpool[{n}-k2s2p0]"
        cov[f"maxpool_bwd_k3s2p1_kernel<{t}>"] = f"test_maxpool[{n}-k3s2p1]"
    cov["bn_finalize_kernel<0, 8>"] = "test_bn_stats_big_integer_maps[fp32-1048576x8]"        # its 8-row tier
    cov["bn_finalize_kernel<0, 32>"] = "test_bn_stats_big_integer_maps[fp32-16384x512]"       # its 16-row tier
    cov["bn_finalize_kernel<1, 8>"] = "test_bn_bwd_accumulate_and_c_valid[fp32-16]"
    cov["bn_finalize_kernel<1, 32>"] = "test_bn_bwd_accumulate_and_c_valid[fp32-264]"
    cov["bn_partial_fold_kernel"] = "test_bn_stats_from_partials[264-6145]"                   # its four-way loop
    cov["rsqrt_eps_kernel"] = "test_bn_eval_invstd[257]"
    return cov


COVERAGE = _table()

_GLOBAL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", re.S)


def _defined():
    """the names of the __global__ functions of conv.hip"""
    return set(_GLOBAL.findall(B.conv_hip_text()))


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
def bn_symbols():
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
        short = _short(s)
        if re.match(r"\w+", short).group(0) in KERNELS:
            out.add(short)
    return out


def _missing_and_stale(symbols, table, unreachable=UNREACHABLE):
    placed = set(table) | set(unreachable)
    return symbols - placed, placed - symbols


def test_every_batchnorm_and_maxpool_kernel_has_a_direct_gpu_case(bn_symbols):
    per_kernel = {}
    for s in bn_symbols:
        k = re.match(r"\w+", s).group(0)
        per_kernel[k] = per_kernel.get(k, 0) + 1
    print(f"BatchNorm / max-pool kernel symbols in the listing ({len(bn_symbols)}): {sorted(per_kernel.items())}")
    assert len(bn_symbols) >= 90, "the listing has fewer of these kernels than it had: the disassembly found too little"
    assert set(per_kernel) == set(KERNELS), f"kernels without any symbol: {sorted(set(KERNELS) - set(per_kernel))}"
    missing, stale = _missing_and_stale(bn_symbols, COVERAGE)
    assert not missing, f"kernels without a direct GPU case in COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE / UNREACHABLE name kernels the library does not have: {sorted(stale)}"
    assert not set(COVERAGE) & set(UNREACHABLE) and all(isinstance(r, str) and r for r in UNREACHABLE.values())


def test_every_global_of_conv_hip_is_placed():
    """a kernel added to conv.hip later goes into KERNELS (and gets a case) or into OUT_OF_SCOPE (and keeps a test elsewhere)"""
    defined = _defined()
    assert defined == set(KERNELS) | OUT_OF_SCOPE, sorted(defined ^ (set(KERNELS) | OUT_OF_SCOPE))
    assert not set(KERNELS) & OUT_OF_SCOPE
    assert {k.split("<")[0] for k in COVERAGE} | {k.split("<")[0] for k in UNREACHABLE} == set(KERNELS)
    assert not [k for k in OUT_OF_SCOPE if re.match(r"(bn_|maxpool_|rsqrt_)", k)]


def _param_sets(fn):
    """[(id, {argname: value})] of a test function's parametrisation, ids as pytest spells them (the mark nearest the
    function first)"""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    per_mark = []
    for m in marks:
        names = [a.strip() for a in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        ids = m.kwargs.get("ids")
        sets = []
        for i, v in enumerate(m.args[1]):
            vals = tuple(v) if len(names) > 1 else (v,)
            if ids is not None:
                ident = ids[i]
            else:
                ident = "-".join(str(x) if isinstance(x, (str, int, float, bool)) or x is None else f"{nm}{i}"
                                 for nm, x in zip(names, vals))
            sets.append((ident, dict(zip(names, vals))))
        per_mark.append(sets)
    out = []
    for combo in itertools.product(*per_mark):
        merged = {}
        for _, d in combo:
            merged.update(d)
        out.append(("-".join(c[0] for c in combo), merged))
    return out


def _case_params(case):
    """(function name, parameter set) of a named case of tests/test_gpu_batchnorm.py; asserts that the case exists"""
    fn_name, ident = re.match(r"^(\w+)\[(.+)\]$", case).groups()
    module = importlib.import_module("tests.test_gpu_batchnorm")
    assert hasattr(module, fn_name), case
    sets = dict(_param_sets(getattr(module, fn_name)))
    assert ident in sets, f"{case}: no such parameter set (has {sorted(sets)[:8]} ...)"
    return fn_name, sets[ident]


def _check_row(sym, case):
    """the named set exists and what it runs is the symbol's instantiation"""
    from tests import test_gpu_batchnorm as T
    back = {v: k for k, v in _T.items()}
    fn, p = _case_params(case)
    m = re.match(r"^(\w+)(?:<(.+)>)?$", sym)
    kernel, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    why = f"{case} does not run {sym}"
    if args and args[0] in back:
        assert p["name"] == back[args[0]], why
        args = args[1:]
    vector_widths = {"test_bn_stats": [p.get("C")], "test_bn_bwd": T.WIDTHS, "test_bn_apply_fwd": T.WIDTHS,
                     "test_stem_bwd": [p.get("C")], "test_stem_fwd": [p.get("C")], "test_maxpool": [16]}
    if kernel == "bn_colstats_kernel":
        want = {"test_bn_stats": ["0", "false", "0"], "test_stem_bwd": ["1", "true", "0"]}.get(fn)
        if fn == "test_bn_bwd":                          # the ReLU is on in every (src, nodres) case: MSRC is the source's
            assert not p["dres"], why
            want = ["1", "false", str(_MSRC[p["src"]])]
        assert want == args and all(c % 8 == 0 for c in vector_widths[fn]), why
        if fn == "test_stem_bwd":
            assert p["hw"][0] % 2 or p["hw"][1] % 2, f"{why}: even maps run the quad kernels"
    elif kernel == "bn_finalize_kernel":
        mode = {"test_bn_stats": 0, "test_bn_stats_big_integer_maps": 0, "test_bn_bwd_accumulate_and_c_valid": 1}.get(fn)
        C = p["shape"][1] if "shape" in p else p["C"]
        assert [str(mode), str(B.finalize_cl(C))] == args, why
    elif kernel == "bn_partial_fold_kernel":
        assert fn == "test_bn_stats_from_partials" and p["parts"] > B.FOLD_ABOVE and B.fold_plan(p["parts"])[2], why
    elif kernel == "rsqrt_eps_kernel":
        assert fn == "test_bn_eval_invstd", why
    elif kernel == "bn_apply_fwd_kernel":
        assert fn == "test_bn_apply_fwd" and [_b(p["res"]), _b(p["mask"])] == args, why
    elif kernel == "bn_apply_bwd_kernel":
        assert fn == "test_bn_bwd" and [str(_MSRC[p["src"]]), _b(p["dres"])] == args, why
    elif kernel in ("bn_apply_bwd_pool_kernel", "bn_colstats_pool_quad_kernel", "bn_apply_bwd_pool_quad_kernel"):
        even = p["hw"][0] % 2 == 0 and p["hw"][1] % 2 == 0
        assert fn == "test_stem_bwd" and even == kernel.endswith("quad_kernel") and p["C"] % 8 == 0, why
    elif kernel == "bn_relu_maxpool_k3s2p1_kernel":
        assert fn == "test_stem_fwd" and p["C"] % 8 == 0, why
    elif kernel in ("bn_colstats_scalar_kernel", "bn_apply_fwd_scalar_kernel", "bn_apply_bwd_scalar_kernel"):
        assert fn == "test_bn_scalar" and p["C"] % 8 != 0 and (kernel != "bn_colstats_scalar_kernel" or args in (["0"], ["1"])), why
    elif kernel in ("maxpool_fwd_kernel", "maxpool_bwd_kernel"):
        assert fn == "test_maxpool_scalar" and p["C"] % 8 != 0, why
    elif kernel == "maxpool_fwd_vec_kernel":
        assert fn == "test_maxpool", why
    elif kernel == "maxpool_bwd_vec_kernel":
        assert fn == "test_maxpool" and tuple(p["pool"]) != (3, 2, 1), why
    else:
        assert kernel == "maxpool_bwd_k3s2p1_kernel" and fn == "test_maxpool" and tuple(p["pool"]) == (3, 2, 1), why


def test_every_named_case_exists_and_runs_the_symbols_instantiation():
    for sym, case in COVERAGE.items():
        _check_row(sym, case)


def test_the_shape_tables_reach_what_they_are_there_for():
    """the widths cover every form of bn_vc and both finalize CL values; the parts tables sit on the boundaries the GPU
    file's docstring names"""
    from tests import test_gpu_batchnorm as T
    assert {B.bn_vc(C) for C in T.WIDTHS} == {1, 2, 8, 18, 11, 32} and B.bn_vc(296) == 1 << B.bn_vc_log2(296) and (296 // 8) % 32
    assert {B.finalize_cl(C) for C in T.WIDTHS} == {8, 32} and {B.finalize_cl(C) for C in T.PARTS} == {8, 32}
    rows, C = T.SHORT_LAST
    parts, rpb = B.bn_parts(rows, C)
    assert rpb > B.ROW_UNROLL * B.row_lanes(C) and rows % rpb and parts > 1
    for C, table in T.PARTS.items():
        PL = 1024 // B.finalize_cl(C)
        assert {1, PL - 1, PL, PL + 1} <= set(table) and max(table) == B.FOLD_ABOVE
        for edge in (3 * PL, 7 * PL):                   # the last parts count below a tier and the first one inside it
            if edge + 1 <= B.FOLD_ABOVE:
                assert {edge, edge + 1} <= set(table)
                assert B.finalize_tiers(edge, 1024 // PL)[0] != B.finalize_tiers(edge + 1, 1024 // PL)[0]
    plans = [B.fold_plan(p) for p in T.FOLD_PARTS]
    assert any(blocks < B.FOLDS for _, blocks, _ in plans) and {four for _, _, four in plans} == {False, True}
    assert (B.fold_plan(6143)[0], B.fold_plan(6145)[0]) == (96, 97)
    assert all(C % 8 for C in T.SCALAR_WIDTHS) and T.MISALIGNED_C % 8 == 0
    assert any(k * k > 9 for k, _, _ in T.POOLS) and (3, 2, 1) in T.POOLS
    assert any(h % 2 == 0 and w % 2 == 0 for h, w in T.STEM_MAPS) and any(h % 2 or w % 2 for h, w in T.STEM_MAPS)
    assert any(3 * (h // 2) * (w // 2) < B.row_lanes(64) for h, w in T.STEM_MAPS)          # fewer quads than row lanes


def test_the_gate_fails_when_a_row_is_deleted_stale_or_mismatched(bn_symbols):
    """the properties the gate exists for, on copies of the table"""
    for key in ("bn_colstats_kernel<float, 1, true, 0>", "bn_finalize_kernel<1, 32>", "bn_partial_fold_kernel",
                "bn_apply_fwd_kernel<_Float16, true, false>", "maxpool_bwd_kernel<std::bfloat16_t>"):
        table = dict(COVERAGE)
        del table[key]
        missing, stale = _missing_and_stale(bn_symbols, table)
        assert missing == {key} and not stale
        assert _missing_and_stale(bn_symbols, table, {key: "a reason"}) == (set(), set())
    table = dict(COVERAGE)
    table["bn_finalize_kernel<0, 16>"] = "test_bn_stats[fp32-8]"                            # no such instantiation
    assert _missing_and_stale(bn_symbols, table) == (set(), {"bn_finalize_kernel<0, 16>"})
    assert _missing_and_stale(bn_symbols, COVERAGE, {"bn_colstats_kernel<float, 0, true, 0>": "never instantiated"})[1]
    for sym, case in (("bn_finalize_kernel<0, 32>", "test_bn_stats[fp32-64]"),               # C = 64 is CL 8
                      ("bn_finalize_kernel<1, 8>", "test_bn_stats[fp32-8]"),                 # the statistics pass is MODE 0
                      ("bn_colstats_kernel<float, 0, false, 0>", "test_bn_stats[bf16-8]"),   # another type
                      ("bn_colstats_kernel<float, 0, false, 0>", "test_bn_stats[fp32-24]"),  # no such set
                      ("bn_colstats_kernel<float, 1, false, 2>", "test_bn_bwd[fp32-y-nodres]"),
                      ("bn_colstats_kernel<float, 1, true, 0>", "test_stem_bwd[fp32-16-12x16]"),      # even: the quad kernels
                      ("bn_apply_bwd_pool_quad_kernel<float>", "test_stem_bwd[fp32-16-9x11]"),
                      ("bn_apply_fwd_kernel<float, true, false>", "test_bn_apply_fwd[fp32-False-True]"),
                      ("bn_apply_bwd_kernel<float, 1, true>", "test_bn_bwd[fp32-y-nodres]"),
                      ("bn_partial_fold_kernel", "test_bn_stats_from_partials[264-256]"),    # 256 partial rows are not folded
                      ("bn_partial_fold_kernel", "test_bn_stats_from_partials[264-6143]"),   # per_block = 96: no four-way trip
                      ("maxpool_bwd_vec_kernel<float>", "test_maxpool[fp32-k3s2p1]"),        # the stem pool has its own kernel
                      ("maxpool_fwd_kernel<float>", "test_maxpool[fp32-k3s2p1]"),            # C = 16: the vector kernel
                      ("bn_apply_fwd_scalar_kernel<float>", "test_bn_stats[fp32-8]")):
        with pytest.raises(AssertionError):
            _check_row(sym, case)
