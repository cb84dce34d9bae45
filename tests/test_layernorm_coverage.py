"""CPU gate on the direct tests of the LayerNorm kernels: every ``ln_fwd_kernel<...>``, ``ln_bwd_kernel<...>``,
``ln_bwd_reduce_kernel<...>`` and ``ln_bwd_reduce_group_kernel`` symbol of the built library is tied to a named parameter set
of tests/test_gpu_layernorm.py whose element types are the symbol's template types and whose width d maps to the symbol's
VPL (cdiv(d, 512), 5..8 -> 8).  Only the names of the listing are read.

``ln_bwd_reduce_kernel`` is defined in csrc/ln_reduce.h, which csrc/layernorm.hip and csrc/attention_cls.hip both include:
each translation unit instantiates it in its own anonymous namespace, the two spell alike in the listing and fold into
one name here.  The name is attributed to the header; the cases named below reach it through ops.layernorm_bwd, and the
instantiation of attention_cls.hip keeps its own test (the ops.attn_cls_bwd case of tests/test_gpu_ops.py)."""
import importlib
import itertools
import os
import re
import sys

import pytest

from tests import rowwise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "data-efficient-video-transformers_amd", "csrc")
SOURCES = ("layernorm.hip", "ln_reduce.h")

_T = {"fp32": "float", "bf16": "std::bfloat16_t", "fp16": "_Float16"}
VPL_WIDTH = {1: 8, 2: 520, 3: 1032, 4: 1544, 8: 2056}            # the smallest d of each VPL among the cases' widths


def vpl_of(d):
    v = -(-d // 512)
    return v if v <= 4 else 8


def bwd_template_types(dy, x, dx, lp):
    """the <TDY, TX, TDX, TL> a case's (dy, x, dx, dx_lp) types are dispatched to: TL is dy's type on the fp32 stream
    (whether or not the 16-bit copy is asked for: one instantiation serves both), and dx's type elsewhere"""
    assert lp in (None, dy)
    return [dy, x, dx, dy if (x == "fp32" and dy != "fp32") else dx]


def _table():
    from tests import test_gpu_layernorm as T
    cov = {}
    for (xn, yn), (vpl, d) in itertools.product(T.FWD_TYPES, VPL_WIDTH.items()):
        cov[f"ln_fwd_kernel<{_T[xn]}, {_T[yn]}, {vpl}>"] = f"test_ln_fwd[{xn}-{yn}-{d}]"
    for (dyn, xn, dxn, lp), (vpl, d) in itertools.product(T.BWD_TYPES, VPL_WIDTH.items()):
        if lp is None:                                              # (the -lp cases run the same instantiation: checked below)
            types = ", ".join(_T[t] for t in bwd_template_types(dyn, xn, dxn, lp))
            cov[f"ln_bwd_kernel<{types}, {vpl}>"] = f"test_ln_bwd[{dyn}-{xn}-{dxn}-{d}]"
    cov["ln_bwd_reduce_kernel<8>"] = "test_ln_bwd_row_counts[512]"              # 128 partial rows
    cov["ln_bwd_reduce_kernel<32>"] = "test_ln_bwd_row_counts[513]"             # 129
    cov["ln_bwd_reduce_group_kernel"] = "test_ln_reduce_group_direct[34]"       # (and test_ln_deferred_reduce through ops)
    return cov


COVERAGE = _table()

_GLOBAL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", re.S)


def _defined():
    """the names of the __global__ functions of layernorm.hip and ln_reduce.h"""
    out = set()
    for f in SOURCES:
        with open(os.path.join(CSRC, f)) as fh:
            out |= set(_GLOBAL.findall(fh.read()))
    return out


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
def ln_symbols():
    """the listing's kernels whose name layernorm.hip or ln_reduce.h defines, without their argument lists"""
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from isa_listing import kernel_listings
    finally:
        sys.path.pop(0)
    names = _defined()
    out = set()
    for s in kernel_listings(dvt_amd._lib.LIB_PATH, demangle=True):
        short = _short(s)
        if re.match(r"\w+", short).group(0) in names:
            out.add(short)
    return out


def _missing_and_stale(symbols, table):
    return symbols - set(table), set(table) - symbols


def test_every_layernorm_kernel_has_a_direct_gpu_case(ln_symbols):
    per_kernel = {}
    for s in ln_symbols:
        k = re.match(r"\w+", s).group(0)
        per_kernel[k] = per_kernel.get(k, 0) + 1
    print(f"LayerNorm kernel symbols in the listing: {sorted(per_kernel.items())}")
    assert len(ln_symbols) >= 60, "the listing has (almost) none of these kernels: the disassembly found nothing"
    missing, stale = _missing_and_stale(ln_symbols, COVERAGE)
    assert not missing, f"LayerNorm kernels without a direct GPU case in COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE names kernels the library does not have: {sorted(stale)}"


def test_every_global_of_the_files_is_accounted_for():
    """a kernel added to layernorm.hip or ln_reduce.h later has to be placed; ln_bwd_reduce_kernel is the header's, and the
    .hip files that instantiate it are the two that include the header"""
    assert _defined() == {k.split("<")[0] for k in COVERAGE}
    with open(os.path.join(CSRC, "ln_reduce.h")) as fh:
        assert set(_GLOBAL.findall(fh.read())) == {"ln_bwd_reduce_kernel"}
    including = set()
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, f)) as fh:
            text = fh.read()
        if f.endswith(".hip") and f != "layernorm.hip":
            assert not set(_GLOBAL.findall(text)) & _defined(), f
        if '#include "ln_reduce.h"' in text:
            including.add(f)
    assert including == {"layernorm.hip", "attention_cls.hip"}


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
    """the parameter set of a named case of tests/test_gpu_layernorm.py; asserts that the case exists"""
    fn_name, ident = re.match(r"^(\w+)\[(.+)\]$", case).groups()
    module = importlib.import_module("tests.test_gpu_layernorm")
    assert hasattr(module, fn_name), case
    sets = dict(_param_sets(getattr(module, fn_name)))
    assert ident in sets, f"{case}: no such parameter set (has {sorted(sets)[:8]} ...)"
    return sets[ident]


def _check_row(sym, case):
    """the named set exists, runs in the symbol's template types and at a width of the symbol's VPL"""
    back = {v: k for k, v in _T.items()}
    p = _case_params(case)
    m = re.match(r"^(\w+)(?:<(.+)>)?$", sym)
    kernel, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    if kernel in ("ln_fwd_kernel", "ln_bwd_kernel"):
        want_types, vpl = [back[a] for a in args[:-1]], int(args[-1])
        types = list(p["types"]) if kernel == "ln_fwd_kernel" else bwd_template_types(*p["types"])
        assert types == want_types, f"{case} runs in {types}, {sym} is instantiated for {want_types}"
        assert all(t in R.DTYPE_ID for t in types)
        assert vpl_of(p["d"]) == vpl, f"{case}: d = {p['d']} is VPL {vpl_of(p['d'])}, {sym} is VPL {vpl}"
    elif kernel == "ln_bwd_reduce_kernel":
        nparts = -(-p["rows"] // 4)
        assert (32 if nparts > 128 else 8) == int(args[0]), f"{case}: {nparts} partial rows do not reach {sym}"
    else:
        assert kernel == "ln_bwd_reduce_group_kernel" and p["count"] > 32


def test_every_named_case_exists_and_runs_the_symbols_instantiation():
    for sym, case in COVERAGE.items():
        _check_row(sym, case)


def test_the_lp_cases_and_every_width_land_on_covered_symbols():
    """every parameter set of the two sweeps maps to a symbol of the table: none of them runs an instantiation the gate
    does not know, and each VPL is met at its smallest and its largest d"""
    from tests import test_gpu_layernorm as T
    for _, p in _param_sets(T.test_ln_fwd):
        assert f"ln_fwd_kernel<{_T[p['types'][0]]}, {_T[p['types'][1]]}, {vpl_of(p['d'])}>" in COVERAGE
    for _, p in _param_sets(T.test_ln_bwd):
        types = ", ".join(_T[t] for t in bwd_template_types(*p["types"]))
        assert f"ln_bwd_kernel<{types}, {vpl_of(p['d'])}>" in COVERAGE
    edges = {1: (8, 512), 2: (520, 1024), 3: (1032, 1536), 4: (1544, 2048), 8: (2056, 4096)}
    for vpl, (lo, hi) in edges.items():
        assert lo in T.WIDTHS and hi in T.WIDTHS and vpl_of(lo) == vpl_of(hi) == vpl and vpl_of(lo - 8) != vpl
    assert {vpl_of(d) for d in T.WIDTHS} == set(edges) and vpl_of(2560) == vpl_of(3584) == 8


def test_the_gate_fails_when_a_row_is_deleted_or_stale(ln_symbols):
    """the properties the gate exists for, on copies of the table"""
    for key in ("ln_fwd_kernel<float, std::bfloat16_t, 3>", "ln_bwd_kernel<_Float16, float, float, _Float16, 8>",
                "ln_bwd_reduce_kernel<32>", "ln_bwd_reduce_group_kernel"):
        table = dict(COVERAGE)
        del table[key]
        missing, stale = _missing_and_stale(ln_symbols, table)
        assert missing == {key} and not stale
    table = dict(COVERAGE)
    table["ln_fwd_kernel<float, float, 5>"] = "test_ln_fwd[fp32-fp32-2056]"                # no such instantiation
    assert _missing_and_stale(ln_symbols, table) == (set(), {"ln_fwd_kernel<float, float, 5>"})
    for sym, case in (("ln_fwd_kernel<float, float, 2>", "test_ln_fwd[fp32-fp32-512]"),      # d = 512 is VPL 1
                      ("ln_fwd_kernel<float, float, 1>", "test_ln_fwd[bf16-fp32-8]"),        # another type
                      ("ln_fwd_kernel<float, float, 1>", "test_ln_fwd[fp32-fp32-16]"),       # no such set
                      ("ln_bwd_reduce_kernel<32>", "test_ln_bwd_row_counts[512]")):          # 128 partial rows: <8>
        with pytest.raises(AssertionError):
            _check_row(sym, case)
