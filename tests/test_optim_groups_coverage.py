"""CPU gate on the direct tests of csrc/optim_groups.hip, after tests/test_optim_coverage.py: every kernel symbol of that
file in the built library -- each mirror type and both kEma forms of the grouped step, and the stand-alone EMA -- is tied to a
named GPU case of tests/test_gpu_optim_groups.py whose mirror has the symbol's type.  Only the names of the listing are read."""
import os
import re
import sys

import pytest

from tests.test_optim_coverage import _GLOBAL, _T, _case_mirror, _short

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "data-efficient-video-transformers_amd", "csrc", "optim_groups.hip")

# kernel -> case, written once per mirror type: {T} the type in the symbol, {m} its id in tests/test_gpu_optim_groups.py
TEMPLATES = [
    ("adamw_groups_kernel<{T}, false>", "test_gpu_optim_groups::test_groups_step_per_group[{m}-workload-0]"),
    ("adamw_groups_kernel<{T}, true>", "test_gpu_optim_groups::test_fused_ema[{m}]"),
]
COVERAGE = {k.format(T=_T[n]): c.format(m=n) for k, c in TEMPLATES for n in _T}
COVERAGE["ema_update_kernel"] = "test_gpu_optim_groups::test_ema_update_exact[0.5]"


def _defined():
    with open(SOURCE) as fh:
        return set(_GLOBAL.findall(fh.read()))


@pytest.fixture(scope="module")
def group_symbols():
    """the listing's kernels whose name optim_groups.hip defines, without their argument lists"""
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


def test_the_file_defines_the_two_kernels_and_optim_hip_none_of_them():
    assert _defined() == {"adamw_groups_kernel", "ema_update_kernel"} == {k.split("<")[0] for k in COVERAGE}
    csrc = os.path.dirname(SOURCE)
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip") and f != "optim_groups.hip":
            with open(os.path.join(csrc, f)) as fh:
                assert not set(_GLOBAL.findall(fh.read())) & _defined(), f


def test_every_kernel_has_a_direct_gpu_case(group_symbols):
    assert len(group_symbols) == 7, sorted(group_symbols)           # 3 mirror types x 2 kEma forms, and the EMA alone
    missing = group_symbols - set(COVERAGE)
    assert not missing, f"kernels of optim_groups.hip without a direct GPU case in COVERAGE: {sorted(missing)}"
    stale = set(COVERAGE) - group_symbols
    assert not stale, f"COVERAGE names kernels the library does not have: {sorted(stale)}"


def test_every_named_case_exists_and_mirrors_in_the_symbols_type():
    back = {v: k for k, v in _T.items()}
    for sym, case in COVERAGE.items():
        mirror = _case_mirror(case)
        m = re.match(r"^\w+<(.+), (?:true|false)>$", sym)
        assert mirror == (back[m.group(1)] if m is not None else "none"), (sym, case, mirror)


def test_the_gate_fails_when_a_row_is_deleted(group_symbols):
    """the property the gate exists for, on a copy of the table"""
    for key in ("ema_update_kernel", "adamw_groups_kernel<_Float16, true>", "adamw_groups_kernel<float, false>"):
        table = dict(COVERAGE)
        del table[key]
        assert key in group_symbols - set(table)
