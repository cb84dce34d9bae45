"""CPU gate on the direct tests of the row, gating, loss, data-movement and LSTM-step kernels: every kernel symbol of those
families in the built library is tied to a named GPU case of tests/test_gpu_rowwise.py, tests/test_gpu_lstm.py,
tests/test_gpu_layernorm.py (the cross-entropy on integer labels) or (cast, add, token assembly, rows_sum)
tests/test_gpu_ops.py whose dtype is the symbol's element type, or is listed as unreachable
through ops with a reason.  Only the names of the listing are read.

A kernel name is attributed to the csrc file that defines it, so the two ``transpose_kernel`` templates (one in an
anonymous namespace of lstm.hip, one of conv.hip; their symbols are spelled alike) are accounted for separately."""
import importlib
import itertools
import os
import re
import sys

import pytest
import torch

from tests import rowwise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "data-efficient-video-transformers_amd", "csrc")

_T = {"fp32": "float", "bf16": "std::bfloat16_t", "fp16": "_Float16"}
_LSTM_ID = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}          # parameter ids of tests/test_gpu_lstm.py
_OPS_ID = {"fp32": "dtype0", "bf16": "dtype1", "fp16": "dtype2"}   # positions in tests/test_gpu_ops.py DTYPES

# (source file, kernel) -> case, written once per element type: {T} the type in the symbol, {n} / {l} / {o} its id in
# tests/test_gpu_rowwise.py / tests/test_gpu_lstm.py / tests/test_gpu_ops.py
TEMPLATES = [
    ("fusion_ssl.hip", "l2norm_fwd_kernel<{T}>", "test_gpu_rowwise::test_l2norm_rows[{n}-1e-12]"),
    ("fusion_ssl.hip", "l2norm_bwd_kernel<{T}>", "test_gpu_rowwise::test_l2norm_rows[{n}-1e-08]"),
    ("fusion_ssl.hip", "cosine_rows_kernel<{T}>", "test_gpu_rowwise::test_cosine_rows[{n}-1e-08]"),
    ("fusion_ssl.hip", "gate_fwd_kernel<{T}>", "test_gpu_rowwise::test_gate[{n}]"),
    ("fusion_ssl.hip", "gate_bwd_kernel<{T}>", "test_gpu_rowwise::test_gate[{n}]"),
    ("elementwise.hip", "add_kernel<{T}>", "test_gpu_rowwise::test_add[{n}]"),
    ("elementwise.hip", "add_rowtable_kernel<{T}>", "test_gpu_rowwise::test_add_rowtable[{n}]"),
    ("elementwise.hip", "copy2d_kernel<{T}>", "test_gpu_rowwise::test_copy2d[{n}-vector]"),
    ("elementwise.hip", "permute021_kernel<{T}>", "test_gpu_rowwise::test_permute_021[{n}]"),
    ("elementwise.hip", "axpby_kernel<{T}>", "test_gpu_rowwise::test_axpby_f32[{n}]"),
    ("elementwise.hip", "act_kernel<{T}, true>", "test_gpu_rowwise::test_act[{n}-gelu]"),
    ("elementwise.hip", "act_kernel<{T}, false>", "test_gpu_rowwise::test_act[{n}-sigmoid]"),
    ("elementwise.hip", "tokens_fwd_kernel<{T}>", "test_gpu_ops::test_tokens_assemble[{o}]"),
    ("elementwise.hip", "tokens_bwd_pos_kernel<{T}>", "test_gpu_rowwise::test_tokens_assemble_bwd[{n}-9-3]"),
    ("elementwise.hip", "strided_rows_sum_kernel<{T}>", "test_gpu_rowwise::test_rows_sum[{n}]"),
    ("elementwise.hip", "few_rows_sum_kernel<{T}>", "test_gpu_rowwise::test_rows_sum[{n}]"),
    ("elementwise.hip", "rows_gather_fwd_kernel<{T}>", "test_gpu_rowwise::test_rows_gather[{n}-0]"),
    ("elementwise.hip", "rows_gather_bwd_kernel<{T}>", "test_gpu_rowwise::test_rows_gather[{n}-1]"),
    ("elementwise.hip", "mean_rows_kernel<{T}, true>", "test_gpu_rowwise::test_mean_rows[{n}]"),
    ("elementwise.hip", "mean_rows_kernel<{T}, false>", "test_gpu_rowwise::test_mean_rows[{n}]"),
    ("losses.hip", "bce_fwd_kernel<{T}>", "test_gpu_rowwise::test_bce_logits[{n}]"),
    ("losses.hip", "bce_bwd_kernel<{T}>", "test_gpu_rowwise::test_bce_logits[{n}]"),
    ("losses.hip", "ce_argmax_kernel<{T}, true>", "test_gpu_rowwise::test_ce_argmax[{n}]"),
    ("losses.hip", "ce_argmax_kernel<{T}, false>", "test_gpu_rowwise::test_ce_argmax[{n}]"),
    ("lstm.hip", "lstm_step_fwd_kernel<{T}>", "test_gpu_lstm::test_forward_step_k_loop_sums_every_group_once[{l}]"),
    ("lstm.hip", "lstm_step_bwd_kernel<{T}>", "test_gpu_lstm::test_lstm_seq_fwd_bwd_direct[{l}-both]"),
    ("lstm.hip", "transpose_kernel<{T}>", "test_gpu_lstm::test_lstm_seq_fwd_bwd_direct[{l}-both]"),
    ("losses.hip", "sigmoid_bce_fwd_kernel<{T}>", "test_gpu_rowwise::test_sigmoid_bce[{n}]"),
    ("losses.hip", "sigmoid_bce_bwd_kernel<{T}>", "test_gpu_rowwise::test_sigmoid_bce[{n}]"),
    ("conv.hip", "transpose_kernel<{T}>", "test_gpu_rowwise::test_transpose_last2[{n}]"),
    ("losses.hip", "ce_labels_fwd_kernel<{T}>", "test_gpu_layernorm::test_ce_labels[{n}]"),
    ("losses.hip", "ce_labels_bwd_kernel<{T}>", "test_gpu_layernorm::test_ce_labels[{n}]"),
]

COVERAGE = {(f, k.format(T=_T[n])): c.format(n=n, l=_LSTM_ID[n], o=_OPS_ID[n]) for f, k, c in TEMPLATES for n in _T}
COVERAGE.update({
    ("losses.hip", "contrastive_rows_fwd_kernel"): "test_gpu_rowwise::test_contrastive_rows[0.1]",
    ("losses.hip", "contrastive_rows_bwd_kernel"): "test_gpu_rowwise::test_contrastive_rows[0.1]",
    ("losses.hip", "mean_kernel"): "test_gpu_rowwise::test_contrastive_rows[0.5]",
})
COVERAGE.update({("elementwise.hip", f"cast_kernel<{_T[s]}, {_T[d]}>"): f"test_gpu_rowwise::test_cast[{s}-{d}]"
                 for s, d in (("fp32", "bf16"), ("fp32", "fp16"), ("bf16", "fp32"), ("fp16", "fp32"), ("fp32", "fp32"),
                              ("bf16", "bf16"), ("fp16", "fp16"))})

UNREACHABLE = {("elementwise.hip", f"tokens_bwd_emb_kernel<{t}>"):
               "ops.tokens_assemble_bwd always asks for dpos, and the positional pass then writes demb as well" for t in _T.values()}

# kernel names in scope, per source file (None: every kernel of the file)
SCOPE = {
    "fusion_ssl.hip": None,
    "elementwise.hip": {"cast_kernel", "add_kernel", "add_rowtable_kernel", "copy2d_kernel", "permute021_kernel", "axpby_kernel",
                        "act_kernel", "tokens_fwd_kernel", "tokens_bwd_emb_kernel", "tokens_bwd_pos_kernel",
                        "strided_rows_sum_kernel", "few_rows_sum_kernel", "rows_gather_fwd_kernel", "rows_gather_bwd_kernel",
                        "mean_rows_kernel"},
    "lstm.hip": {"lstm_step_fwd_kernel", "lstm_step_bwd_kernel", "transpose_kernel"},
    "losses.hip": {"bce_fwd_kernel", "bce_bwd_kernel", "ce_argmax_kernel", "sigmoid_bce_fwd_kernel", "sigmoid_bce_bwd_kernel",
                   "contrastive_rows_fwd_kernel", "contrastive_rows_bwd_kernel", "mean_kernel", "ce_labels_fwd_kernel",
                   "ce_labels_bwd_kernel"},
    "conv.hip": {"transpose_kernel"},
}
# the other kernels of elementwise.hip have tests of their own in tests/test_gpu_ops.py (dropout)
ELEMENTWISE_ELSEWHERE = {"dropout_kernel", "dropout_fused_kernel", "rng_advance_kernel"}
# every kernel of losses.hip is in scope (the cross-entropy on integer labels: the cases of tests/test_gpu_layernorm.py)
LOSSES_ELSEWHERE = set()

_GLOBAL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", re.S)


def _defined_in():
    """kernel name -> the csrc files that define a __global__ function of that name"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            with open(os.path.join(CSRC, f)) as fh:
                for name in set(_GLOBAL.findall(fh.read())):
                    out.setdefault(name, set()).add(f)
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


def _in_scope(fname, base):
    return fname in SCOPE and (SCOPE[fname] is None or base in SCOPE[fname])


@pytest.fixture(scope="module")
def rowwise_symbols():
    """{(source file, symbol)} of the listing's kernels whose name a file of SCOPE defines and has in scope"""
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from isa_listing import kernel_listings
    finally:
        sys.path.pop(0)
    where = _defined_in()
    out = set()
    for s in kernel_listings(dvt_amd._lib.LIB_PATH, demangle=True):
        short = _short(s)
        base = re.match(r"\w+", short).group(0)
        for f in where.get(base, ()):
            if _in_scope(f, base):
                out.add((f, short))
    return out


def test_every_rowwise_kernel_has_a_direct_gpu_case(rowwise_symbols):
    assert len(rowwise_symbols) > 100, "the listing has (almost) none of these kernels: the disassembly found nothing"
    missing = rowwise_symbols - set(COVERAGE) - set(UNREACHABLE)
    assert not missing, f"kernels without a direct GPU case in COVERAGE (or a reason in UNREACHABLE): {sorted(missing)}"
    stale = (set(COVERAGE) | set(UNREACHABLE)) - rowwise_symbols
    assert not stale, f"COVERAGE / UNREACHABLE name kernels the library does not have: {sorted(stale)}"
    assert not set(COVERAGE) & set(UNREACHABLE)


def test_scope_accounts_for_every_kernel_of_its_files():
    """both transpose_kernel definitions are seen, every kernel of elementwise.hip is either in scope or known to be tested
    elsewhere, and a kernel added to one of the files has to be placed"""
    where = _defined_in()
    assert where["transpose_kernel"] == {"lstm.hip", "conv.hip"}
    assert {k for k, fs in where.items() if "elementwise.hip" in fs} == SCOPE["elementwise.hip"] | ELEMENTWISE_ELSEWHERE
    assert {k for k, fs in where.items() if "losses.hip" in fs} == SCOPE["losses.hip"] | LOSSES_ELSEWHERE
    for f, names in SCOPE.items():
        for k in names or ():
            assert f in where.get(k, ()), f"{f} defines no kernel {k}"
    assert {k for k, fs in where.items() if "fusion_ssl.hip" in fs} == {k.split("<")[0] for f, k in COVERAGE if f == "fusion_ssl.hip"}


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


_TORCH_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def _case_types(case):
    """the element types (names of rowwise_ref.DTYPES) a named case runs in; asserts that the case exists"""
    mod, rest = case.split("::")
    fn_name, ident = re.match(r"^(\w+)\[(.+)\]$", rest).groups()
    module = importlib.import_module(f"tests.{mod}")
    assert hasattr(module, fn_name), case
    sets = dict(_param_sets(getattr(module, fn_name)))
    assert ident in sets, f"{case}: no such parameter set (has {sorted(sets)[:8]} ...)"
    p = sets[ident]
    if "src" in p and "dst" in p:
        return [p["src"], p["dst"]]
    if "name" in p:
        return [p["name"]]
    if "dtype" in p:
        return [_TORCH_NAME[p["dtype"]]]
    return ["fp32"]                                        # (the contrastive kernels: float only)


def test_every_named_case_exists_and_runs_in_the_symbols_type():
    back = {v: k for k, v in _T.items()}
    for (f, sym), case in COVERAGE.items():
        types = _case_types(case)
        m = re.match(r"^\w+<(.+)>$", sym)
        want = ["fp32"] if m is None else [back[a.strip()] for a in m.group(1).split(",") if a.strip() in back]
        assert types == want, f"{case} runs in {types}, {sym} of {f} is instantiated for {want}"
        assert all(R.DTYPE_ID[t] in (0, 1, 2) for t in types)


def test_the_gate_fails_when_a_row_is_deleted(rowwise_symbols):
    """the property the gate exists for, on a copy of the table"""
    for key in (("conv.hip", "transpose_kernel<float>"), ("lstm.hip", "transpose_kernel<float>"),
                ("fusion_ssl.hip", "cosine_rows_kernel<_Float16>")):
        table = dict(COVERAGE)
        del table[key]
        assert key in rowwise_symbols - set(table) - set(UNREACHABLE)
