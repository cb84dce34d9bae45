"""CPU gate on the mixed-shape MFMA hazard (tools/check_mfma_hazards.py): the built library keeps every dependent pair of a
16x16x32 and a 16x16x16 MFMA past the margin, the check does flag the unfenced window forward, every kernel that mixes the
two shapes has an exact GPU case (tests/test_gpu_mfma_exact.py), and those cases would see a missing k-step."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from tests import mfma_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every kernel of the library that mixes MFMA opcodes on one accumulator -> the exact GPU case that launches it
MIXING_COVERAGE = {
    "conv3x1_fwd_pipe_kernel<std::bfloat16_t, 1>": "test_window_forward_exact[pipe1-bf16]",
    "conv3x1_fwd_pipe_kernel<std::bfloat16_t, 2>": "test_window_forward_exact[pipe2-bf16]",
    "conv3x1_fwd_pipe_kernel<std::bfloat16_t, 3>": "test_window_forward_exact[pipe3-bf16]",
    "conv3x1_fwd_pipe_kernel<_Float16, 1>": "test_window_forward_exact[pipe1-fp16]",
    "conv3x1_fwd_pipe_kernel<_Float16, 2>": "test_window_forward_exact[pipe2-fp16]",
    "conv3x1_fwd_pipe_kernel<_Float16, 3>": "test_window_forward_exact[pipe3-fp16]",
    "conv3x1_fwd_kernel<std::bfloat16_t, 4>": "test_window_forward_exact[plain4-bf16]",
    "conv3x1_fwd_kernel<std::bfloat16_t, 5>": "test_window_forward_exact[plain5-bf16]",
    "conv3x1_fwd_kernel<std::bfloat16_t, 6>": "test_window_forward_exact[plain6-bf16]",
    "conv3x1_fwd_kernel<_Float16, 4>": "test_window_forward_exact[plain4-fp16]",
    "conv3x1_fwd_kernel<_Float16, 5>": "test_window_forward_exact[plain5-fp16]",
    "conv3x1_fwd_kernel<_Float16, 6>": "test_window_forward_exact[plain6-fp16]",
    "conv3x3_stream_kernel<std::bfloat16_t, 144, 64, 9, 0>": "test_stream_conv3x3_exact[144to64-bf16]",
    "conv3x3_stream_kernel<_Float16, 144, 64, 9, 0>": "test_stream_conv3x3_exact[144to64-fp16]",
    "conv3x3_stream_kernel<std::bfloat16_t, 288, 64, 9, 0>": "test_stream_conv3x3_exact[288to128-bf16]",
    "conv3x3_stream_kernel<_Float16, 288, 64, 9, 0>": "test_stream_conv3x3_exact[288to128-fp16]",
}
_DNAME = {"std::bfloat16_t": "bf16", "_Float16": "fp16"}
_WIN = re.compile(r"^conv3x1_fwd(_pipe)?_kernel<(std::bfloat16_t|_Float16), (\d+)>$")


def _tool():
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def product_scan():
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    return _tool().scan(dvt_amd._lib.LIB_PATH)


def _expected_mixing(so_path):
    """kernels with both MFMA shapes, read straight from the listing (no dataflow): the ones the scan must report"""
    tool = _tool()
    from isa_listing import kernel_listings                  # (tools/, on the path once the tool is loaded)
    out = set()
    for sym, insns in kernel_listings(so_path, demangle=True).items():
        ops = {t.split()[0] for _, t in insns if t.startswith("v_mfma")}
        if any("16x16x32" in o for o in ops) and any("16x16x16" in o for o in ops):
            out.add(tool.short_name(sym))
    return out


def test_product_library_keeps_every_mixed_shape_pair_past_the_margin(product_scan):
    import dvt_amd
    expected = _expected_mixing(dvt_amd._lib.LIB_PATH)
    assert expected, "the listing has no kernel with both MFMA shapes: the disassembly found nothing"
    assert set(product_scan) == expected
    tool = _tool()
    bad = tool.violations(product_scan)
    assert not bad, f"dependent MFMAs of two shapes below the margin: {bad}"
    # the listing's branches resolve into loops (a change of the disassembler's branch format must not turn the CFG into a DAG)
    from isa_listing import kernel_listings
    loops = {tool.short_name(k): tool.back_edges(v) for k, v in kernel_listings(dvt_amd._lib.LIB_PATH, demangle=True).items()}
    assert all(loops[k] >= 1 for k in product_scan), {k: loops[k] for k in product_scan}
    for name, (mixing, _) in product_scan.items():        # both transitions, 16x16x32 -> 16x16x16 and back, were seen
        assert sorted(("16x16x32" in a, "16x16x16" in b) for a, b in mixing) == [(False, False), (True, True)], (name, mixing)


def test_unfenced_window_forward_is_flagged(tmp_path):
    """Negative control: csrc/conv3x1_fwd.hip without its fence (-DDVT_NO_MFMA_SHAPE_FENCE), with the library's own flags:
    exactly the instantiations of fewer than four position blocks per wave (0 - 2 MFMAs between the shapes) are flagged."""
    sys.path.insert(0, os.path.join(ROOT, "data-efficient-video-transformers_amd"))
    try:
        import build as B
        hipcc = B._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    finally:
        sys.path.pop(0)
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    obj = str(tmp_path / "conv3x1_fwd_nofence.o")
    subprocess.run([hipcc, *B.FLAGS, "-DDVT_NO_MFMA_SHAPE_FENCE", "-c", os.path.join(B.CSRC, "conv3x1_fwd.hip"), "-o", obj],
                   check=True, capture_output=True)
    tool = _tool()
    rep = tool.scan(obj)
    windows = {k: _WIN.match(k) for k in rep if _WIN.match(k)}
    assert {int(m.group(3)) for m in windows.values()} == {1, 2, 3, 4, 5, 6}
    flagged = set(tool.violations(rep))
    assert flagged == {k for k, m in windows.items() if int(m.group(3)) <= 3}
    for d in ("std::bfloat16_t", "_Float16"):
        for npb in (1, 2, 3):
            assert f"conv3x1_fwd_pipe_kernel<{d}, {npb}>" in flagged


def test_every_mixing_kernel_has_an_exact_gpu_case(product_scan):
    """The coverage table lists exactly the mixing kernels, and each listed case launches its kernel: the window forward's
    choice of instantiation is the library's own (dvt_conv3x1_fwd_plan), the streamed kernel's follows its channel pair."""
    from tests import test_gpu_mfma_exact as G
    from dvt_amd import ops
    missing = set(product_scan) - set(MIXING_COVERAGE)
    assert not missing, f"kernels mixing MFMA shapes without an exact GPU case in MIXING_COVERAGE: {sorted(missing)}"
    assert set(MIXING_COVERAGE) == set(product_scan), "MIXING_COVERAGE lists kernels that no longer mix MFMA shapes"
    import dvt_amd
    lib = dvt_amd._lib.load()
    for sym, case in MIXING_COVERAGE.items():
        fn, cid, dname = re.match(r"^(\w+)\[(\w+)-(\w+)\]$", case).groups()
        assert hasattr(G, fn), case
        dtype = G.DTYPES[dname]
        m = _WIN.match(sym)
        if m:
            assert fn == "test_window_forward_exact" and dname == _DNAME[m.group(2)], sym
            (N, T, H, W), form = G.WINDOW_CASES[cid]
            assert ops.conv3x1_fwd_plan(N, T, H * W, dtype) == form == (int(m.group(3)), m.group(1) is not None), sym
        else:
            m = re.match(r"^conv3x3_stream_kernel<(std::bfloat16_t|_Float16), (\d+), (\d+), 9, 0>$", sym)
            assert m and fn == "test_stream_conv3x3_exact" and dname == _DNAME[m.group(1)], sym
            Cin, Cout, N, H, W = G.STREAM_CASES[cid]
            # one launch per group of int(m.group(3)) output channels (dvt_conv3x3_stream: 288 -> 128 as two 288 -> 64 halves)
            assert Cin == int(m.group(2)) and Cout in (int(m.group(3)), 2 * int(m.group(3))), sym
            dt = dvt_amd._lib.BF16 if dname == "bf16" else dvt_amd._lib.F16
            assert lib.dvt_conv3x3_stream_supported(N, H, W, Cin, Cout, dt) == 1, sym


def test_window_forward_plan_matches_the_built_forms():
    """The launcher takes 1 - 3 position blocks per wave with helper waves and 4 - 6 without, over many clip geometries; the
    query refuses what dvt_conv3x1_fwd_supported refuses and validates its outputs before anything else."""
    import ctypes
    import dvt_amd
    from dvt_amd import ops
    lib = dvt_amd._lib.load()
    seen = set()
    for T in range(1, 100):
        for Lp in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 20, 28, 49, 56, 196, 784, 3136, 720720):
            plan = ops.conv3x1_fwd_plan(2, T, Lp, torch.bfloat16)
            assert (plan is not None) == bool(lib.dvt_conv3x1_fwd_supported(2, T, Lp, 144, 64, dvt_amd._lib.BF16))
            if plan is not None:
                assert plan[1] == (plan[0] <= 3), (T, Lp, plan)
                seen.add(plan)
    assert seen == {(1, True), (2, True), (3, True), (4, False), (5, False), (6, False)}
    assert ops.conv3x1_fwd_plan(2, 12, 49, torch.bfloat16) is None            # no segment length divides 49 -> refused
    npb, pipe = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.dvt_conv3x1_fwd_plan(2, 12, 64, 64, 64, dvt_amd._lib.BF16, ctypes.byref(npb), ctypes.byref(pipe)) == 0
    assert (npb.value, pipe.value) == (0, 0)                                  # (the 64-channel form has no blocks to report)
    assert lib.dvt_conv3x1_fwd_plan(2, 12, 64, 144, 64, dvt_amd._lib.BF16, None, ctypes.byref(pipe)) == -1


def _pairs(listing):
    tool = _tool()
    insns = [(4 * i, t) for i, t in enumerate(listing)]
    return tool.kernel_report(insns)


def test_scan_takes_the_minimum_over_paths_and_loops():
    """The dataflow on small listings: a loop's back edge, the shorter of two paths, AGPR ranges, partial overlap of one
    opcode, wait states of s_nop, the nearest writer only."""
    m32, m16 = "v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x16_bf16"
    # loop: the 16x16x16 at the bottom feeds the 16x16x32 at the top through the back edge.  Branches are written as
    # llvm-objdump prints them: simm16 in dwords from the next instruction, unsigned (65532 = -4: to the top of four)
    loop = [f"{m32} v[0:3], v[8:11], v[12:15], v[0:3]", f"{m32} v[4:7], v[8:11], v[12:15], v[4:7]",
            f"{m16} v[0:3], v[8:9], v[12:13], v[0:3]", "s_cbranch_scc1 65532"]
    tool = _tool()
    assert tool.back_edges([(4 * i, t) for i, t in enumerate(loop)]) == 1
    mixing, bad = _pairs(loop)
    # (wait states, MFMAs) between: 32 -> 16 one MFMA; 16 -> 32 across the edge only the branch
    assert sorted((b[4], b[5]) for b in bad) == [(1, 0), (1, 1)]
    mixing, bad = _pairs(loop[:3] + ["s_nop 15", "s_cbranch_scc1 65531"])         # a fence on the back edge path only
    assert [(b[4], b[5]) for b in bad] == [(1, 1)] and "16x16x16" in bad[0][3]
    mixing, bad = _pairs(loop[:2] + ["s_nop 15"] + loop[2:3] + ["s_nop 15", "s_cbranch_scc1 65530"])
    assert not bad and mixing == {("f32_16x16x32_bf16", "f32_16x16x16_bf16"): (17, 1),
                                  ("f32_16x16x16_bf16", "f32_16x16x32_bf16"): (17, 0)}
    with pytest.raises(ValueError):
        _pairs(loop[:3] + ["s_cbranch_scc1 65000"])                           # a target outside the kernel
    # two paths from the writer to the reader: 20 wait states or 2; the short one decides
    fork = [f"{m32} a[0:3], v[8:11], v[12:15], a[0:3]", "s_cbranch_vccz 2", "s_nop 15", "s_nop 3",
            f"{m16} a[0:3], v[8:9], v[12:13], a[0:3]", "s_endpgm"]
    mixing, bad = _pairs(fork)
    assert [(b[4], b[5]) for b in bad] == [(1, 0)]
    assert not _pairs(fork[:1] + fork[2:])[1]                                     # without the branch: 20 states
    # one opcode: exact overlap is the interlocked case, partial overlap is not; VGPRs and AGPRs are different registers
    assert not _pairs([f"{m32} v[0:3], v[8:11], v[12:15], v[0:3]", f"{m32} v[0:3], v[8:11], v[12:15], v[0:3]"])[0]
    assert len(_pairs([f"{m32} v[0:3], v[8:11], v[12:15], v[0:3]", f"{m32} v[2:5], v[8:11], v[12:15], v[2:5]"])[1]) == 1
    assert not _pairs([f"{m32} v[0:3], v[8:11], v[12:15], v[0:3]", f"{m16} a[0:3], v[8:9], v[12:13], a[0:3]"])[0]
    # a later writer of the same registers is the producer: the 16x16x16 reads the second 16x16x32's result, three apart
    near = [f"{m32} v[0:3], v[8:11], v[12:15], 0", f"{m32} v[0:3], v[8:11], v[12:15], 0",
            f"{m32} v[4:7], v[8:11], v[12:15], 0", f"{m32} v[16:19], v[8:11], v[12:15], 0",
            f"{m32} v[20:23], v[8:11], v[12:15], 0", f"{m16} v[0:3], v[8:9], v[12:13], v[0:3]"]
    mixing, bad = _pairs(near)
    assert not bad and mixing == {("f32_16x16x32_bf16", "f32_16x16x16_bf16"): (3, 3)}


def _sensitive(x, w, ranges, padding, bound):
    """the float64 k-step restatement sums to the convolution, the sums are exact integers within `bound`, and dropping any
    single k-step changes at least one output"""
    full = torch.nn.functional.conv2d(x, w, None, 1, padding)
    parts = X.kstep_partials(x, w, ranges, padding)
    assert torch.equal(sum(p for _, _, p in parts), full)
    assert torch.equal(full, full.round()) and full.abs().max() <= bound
    for tap, r, p in parts:
        assert not torch.equal(full - p, full), f"dropping tap {tap}, range {ranges[r]} changes no output"
    return full, parts


@pytest.mark.parametrize("case", ["pipe1", "pipe3", "plain4", "plain6"])
def test_window_exact_operands_see_every_missing_kstep(case):
    from tests import test_gpu_mfma_exact as G
    (N, T, H, W), _ = G.WINDOW_CASES[case]
    Lp = H * W
    x = X.one_hot_input(N * T * Lp, 144, X.WINDOW_RANGES, seed=T * 100 + Lp).view(N, T, Lp, 144).permute(0, 3, 1, 2)
    full, parts = _sensitive(x, X.window_weights(), X.WINDOW_RANGES, (1, 0), 256)
    assert len(parts) == 3 * 5
    if T >= 3:                                         # an interior frame: the 15 steps weigh 1 .. 15, each a different amount
        for co in (0, 7, 63):
            amounts = sorted(int(p[0, co, 1, 0]) for _, _, p in parts)
            assert amounts == list(range(1, 16))


@pytest.mark.parametrize("cin,cout", [(144, 64), (288, 128)])
def test_stream_exact_operands_see_every_missing_kstep(cin, cout):
    x = X.one_hot_input(2 * 6 * 7, cin, X.stream_ranges(cin), seed=cin).view(2, 6, 7, cin).permute(0, 3, 1, 2)
    full, parts = _sensitive(x, X.stream_weights(cin, cout), X.stream_ranges(cin), 1, 256)
    assert len(parts) == 9 * (cin // 48) * 2
