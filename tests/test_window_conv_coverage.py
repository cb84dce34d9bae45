"""CPU gate on the exact tests of the LDS-window convolutions: every conv3x3_c64[_wgrad]_kernel, conv3x3_stream_kernel,
conv3x1_{fwd, fwd_pipe, c64, dbn, wgrad, wgrad_pipe}_kernel and conv_stem_kernel symbol of the built library is launched by a
named case of tests/test_gpu_window_conv_exact.py (the 16 symbols that mix MFMA shapes: of tests/test_gpu_mfma_exact.py) --
the library's own plan queries say that case takes that instantiation -- or is listed as unreachable with a reason that a
plan sweep confirms; every reference stays in the exact range of both 16-bit types and of fp32 sums; and the operands of
every case see a dropped, doubled or misplaced piece.

Not exact anywhere: the training-mode correction of the fused BatchNorm backward (MODE 2 of conv3x1_dbn_kernel and of the
stream fallback with training = 1) divides by the row count, which is no power of two for the NB = 6 and fallback geometries;
it stays with test_fused_mid_batchnorm_backward_against_fp32_autograd and
test_temporal_data_gradient_with_the_mid_batchnorm_backward_fused (tests/test_gpu_cnn.py).  Its data path -- window, taps,
staging, z rows, mask, stores -- is the eval-mode one, which is exact here.
"""
import re

import pytest
import torch

from tests import conv_exact as V
from tests import gemm_exact as X
from tests import test_gpu_mfma_exact as GM
from tests import test_gpu_window_conv_exact as G
from tests.test_gemm_coverage import _short
from tests.test_isa_hazards import MIXING_COVERAGE

_T = {"bf16": "std::bfloat16_t", "fp16": "_Float16"}

# every kernel symbol of the family -> the exact GPU case that launches it
_FAMILY = re.compile(r"^(conv3x3_c64(_wgrad)?_kernel|conv3x3_stream_kernel|conv3x1_(fwd|fwd_pipe|c64|dbn|wgrad|wgrad_pipe)_kernel|"
                     r"conv_stem_kernel)<.*>$")
# the family's symbols that mix MFMA shapes: conv3x1_fwd[_pipe]_kernel, conv3x3_stream_kernel<., 144 | 288, 64, 9, 0>
WINDOW_COVERAGE = {s: c for s, c in MIXING_COVERAGE.items() if _FAMILY.match(s)}
assert len(WINDOW_COVERAGE) == 16
for _d, _e in _T.items():
    WINDOW_COVERAGE[f"conv3x3_c64_kernel<{_e}>"] = f"test_conv3x3_c64_exact[persist_8x8-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_stream_kernel<{_e}, 64, 144, 9, 0>"] = f"test_conv3x3_stream_exact[64to144_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_stream_kernel<{_e}, 128, 144, 9, 0>"] = f"test_conv3x3_stream_exact[128to288_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_stream_kernel<{_e}, 64, 144, 3, 0>"] = f"test_conv3x1_stream_exact[ragged_5x112-{_d}]"
    for _m in (1, 2):
        WINDOW_COVERAGE[f"conv3x3_stream_kernel<{_e}, 64, 144, 3, {_m}>"] = f"test_conv3x1_bn_bwd_exact[stream_ragged-{_d}]"
        for _nb in (2, 4, 6):
            WINDOW_COVERAGE[f"conv3x1_dbn_kernel<{_e}, {_nb}, {_m}>"] = f"test_conv3x1_bn_bwd_exact[nb{_nb}_persist-{_d}]"
    for _n in range(1, 7):
        WINDOW_COVERAGE[f"conv3x1_c64_kernel<{_e}, {_n}>"] = f"test_conv3x1_c64_exact[npb{_n}_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x1_wgrad_kernel<{_e}>"] = f"test_conv3x1_wgrad_exact[plain_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x1_wgrad_pipe_kernel<{_e}>"] = f"test_conv3x1_wgrad_exact[pipe_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_c64_wgrad_kernel<{_e}, 4>"] = f"test_conv3x3_c64_wgrad_exact[mb4_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_c64_wgrad_kernel<{_e}, 5>"] = f"test_conv3x3_c64_wgrad_exact[mb5_persist-{_d}]"
    WINDOW_COVERAGE[f"conv3x3_c64_wgrad_kernel<{_e}, 1>"] = f"test_conv3x3_c64_wgrad_exact[mb1_persist-{_d}]"
    WINDOW_COVERAGE[f"conv_stem_kernel<{_e}>"] = f"test_conv_stem_exact[ragged_odd-{_d}]"

# symbol -> one sentence why no call reaches it (none today: every instantiation of the family is planned for some geometry)
UNREACHABLE = {}


@pytest.fixture(scope="module")
def window_symbols():
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


# ---------------------------------------------------------------- symbols from the plan queries (no device)
def _lib():
    import dvt_amd
    return dvt_amd._lib.load(), dvt_amd._lib


def _dt(dtype):
    from dvt_amd import ops
    return ops._DT[dtype]


def sym_c64(N, H, W, dtype, e):
    return {f"conv3x3_c64_kernel<{e}>"} if _lib()[0].dvt_conv3x3_c64_supported(N, H, W, _dt(dtype)) else set()


def sym_stream(N, H, W, Cin, Cout, dtype, e):
    from dvt_amd import ops
    p = ops.conv3x3_stream_plan(N, H, W, Cin, Cout, dtype)
    return {f"conv3x3_stream_kernel<{e}, {p.ci}, {p.co}, 9, 0>"} if p else set()


def sym_stream31(N, T, Lp, dtype, e):
    return {f"conv3x3_stream_kernel<{e}, 64, 144, 3, 0>"} if _lib()[0].dvt_conv3x1_stream_supported(N, T, Lp, 64, 144, _dt(dtype)) else set()


def sym_win64(N, T, Lp, dtype, e):
    from dvt_amd import ops
    n = ops.conv3x1_c64_plan(N, T, Lp, dtype)
    return {f"conv3x1_c64_kernel<{e}, {n}>"} if n else set()


def sym_win144(N, T, Lp, dtype, e):
    from dvt_amd import ops
    p = ops.conv3x1_fwd_plan(N, T, Lp, dtype)
    return {f"conv3x1_fwd{'_pipe' if p[1] else ''}_kernel<{e}, {p[0]}>"} if p else set()


def sym_stem(N, H, Wp, dtype, e):
    return {f"conv_stem_kernel<{e}>"} if _lib()[0].dvt_conv_stem7_supported(N, H, Wp, _dt(dtype)) else set()


def sym_wgrad33(N, H, W, Cout, dtype, e):
    from dvt_amd import ops
    return {f"conv3x3_c64_wgrad_kernel<{e}, {mb}>" for _, _, mb in ops.conv3x3_c64_wgrad_plan(N, H, W, Cout, dtype) or ()}


def sym_wgrad31(N, T, Lp, dtype, e):
    from dvt_amd import ops
    p = ops.conv3x1_wgrad_plan(N, T, Lp, dtype)
    return set() if p is None else {f"conv3x1_wgrad{'_pipe' if p else ''}_kernel<{e}>"}


def sym_bn_bwd(N, T, Lp, dtype, e):
    from dvt_amd import ops
    p = ops.conv3x1_stream_bn_bwd_plan(N, T, Lp, dtype)
    if p is None:
        return set()
    if p.kernel == "window":
        return {f"conv3x1_dbn_kernel<{e}, {p.nb}, {m}>" for m in (1, 2)}
    return {f"conv3x3_stream_kernel<{e}, 64, 144, 3, {m}>" for m in (1, 2)}


def _case_symbols(case):
    """the symbols a named GPU case launches, from the library's plan queries; the plan the case asserts on the GPU is
    checked here too"""
    from dvt_amd import ops
    fn, name, dname = re.match(r"^(\w+)\[(\w+)-(\w+)\]$", case).groups()
    mod = G if hasattr(G, fn) else GM
    assert hasattr(mod, fn) and dname in mod.DTYPES, case
    dtype, e = mod.DTYPES[dname], _T[dname]
    if fn == "test_conv3x3_c64_exact":
        return sym_c64(*G.C64_CASES[name], dtype, e)
    if fn == "test_conv3x3_stream_exact":
        (Cin, Cout, N, H, W), inst = G.STREAM_CASES[name]
        assert ops.conv3x3_stream_plan(N, H, W, Cin, Cout, dtype) == inst, case
        return sym_stream(N, H, W, Cin, Cout, dtype, e)
    if fn == "test_conv3x1_stream_exact":
        N, T, H, W = G.STREAM31_CASES[name]
        return sym_stream31(N, T, H * W, dtype, e)
    if fn == "test_conv3x1_c64_exact":
        (N, T, H, W), npb = G.WIN64_CASES[name]
        assert ops.conv3x1_c64_plan(N, T, H * W, dtype) == npb, case
        return sym_win64(N, T, H * W, dtype, e)
    if fn == "test_conv_stem_exact":
        return sym_stem(*G.STEM_CASES[name], dtype, e)
    if fn == "test_conv3x3_c64_wgrad_exact":
        (N, H, W, Cout), launches = G.WGRAD33_CASES[name]
        assert ops.conv3x3_c64_wgrad_plan(N, H, W, Cout, dtype) == launches, case
        return sym_wgrad33(N, H, W, Cout, dtype, e)
    if fn == "test_conv3x1_wgrad_exact":
        (N, T, H, W), pipe = G.WGRAD31_CASES[name]
        assert ops.conv3x1_wgrad_plan(N, T, H * W, dtype) is pipe, case
        return sym_wgrad31(N, T, H * W, dtype, e)
    if fn == "test_conv3x1_bn_bwd_exact":
        (N, T, H, W), plan = G.DBN_CASES[name]
        assert ops.conv3x1_stream_bn_bwd_plan(N, T, H * W, dtype) == plan, case
        return sym_bn_bwd(N, T, H * W, dtype, e)
    if fn == "test_window_forward_exact":
        (N, T, H, W), form = GM.WINDOW_CASES[name]
        assert ops.conv3x1_fwd_plan(N, T, H * W, dtype) == form, case
        return sym_win144(N, T, H * W, dtype, e)
    if fn == "test_stream_conv3x3_exact":
        Cin, Cout, N, H, W = GM.STREAM_CASES[name]
        return sym_stream(N, H, W, Cin, Cout, dtype, e)
    raise AssertionError(f"unknown case {case}")


def _all_cases():
    for fn, cases in (("test_conv3x3_c64_exact", G.C64_CASES), ("test_conv3x3_stream_exact", G.STREAM_CASES),
                      ("test_conv3x1_stream_exact", G.STREAM31_CASES), ("test_conv3x1_c64_exact", G.WIN64_CASES),
                      ("test_conv_stem_exact", G.STEM_CASES), ("test_conv3x3_c64_wgrad_exact", G.WGRAD33_CASES),
                      ("test_conv3x1_wgrad_exact", G.WGRAD31_CASES), ("test_conv3x1_bn_bwd_exact", G.DBN_CASES)):
        for name in cases:
            for dname in G.DTYPES:
                yield f"{fn}[{name}-{dname}]"


def test_every_window_kernel_has_an_exact_gpu_case(window_symbols):
    assert len(window_symbols) >= 60, "the listing has (almost) no window convolution kernels: the disassembly found nothing"
    missing = window_symbols - set(WINDOW_COVERAGE) - set(UNREACHABLE)
    assert not missing, f"window convolution kernels without an exact GPU case in WINDOW_COVERAGE (or a reason in UNREACHABLE): {sorted(missing)}"
    stale = (set(WINDOW_COVERAGE) | set(UNREACHABLE)) - window_symbols
    assert not stale, f"WINDOW_COVERAGE / UNREACHABLE name symbols the library does not have: {sorted(stale)}"
    assert not set(WINDOW_COVERAGE) & set(UNREACHABLE)
    assert all(isinstance(r, str) and r.count(".") <= 1 and len(r) > 20 for r in UNREACHABLE.values())


def test_every_covered_kernel_is_what_its_case_launches():
    cache = {}
    for sym, case in WINDOW_COVERAGE.items():
        if case not in cache:
            cache[case] = _case_symbols(case)
        assert sym in cache[case], f"{case} launches {sorted(cache[case])}, not {sym}"


def test_every_case_states_the_plan_the_library_reports():
    """every named case, covered symbol or not, launches a kernel of the family and names the instantiation the query reports
    (so a case whose expectation is wrong fails here, without a GPU); and the shapes are what their names say: `ragged` / `few`
    cases have fewer tiles than 256 workgroups; `persist` ones more than BUFFERS x 256, so that a workgroup of the persistent
    grid fills every LDS buffer of the kernel and wraps back to the first while the last round is partial -- and, where
    BatchNorm partial rows are checked, at most 3 x 256 (the bound of G.check_partial_bound)"""
    for case in _all_cases():
        syms = _case_symbols(case)
        assert syms and syms <= set(WINDOW_COVERAGE), (case, syms)
    for fam, cases in (("c64", G.C64_CASES), ("stream", G.STREAM_CASES), ("stream31", G.STREAM31_CASES), ("win64", G.WIN64_CASES),
                       ("stem", G.STEM_CASES), ("wgrad33", G.WGRAD33_CASES), ("wgrad31", G.WGRAD31_CASES), ("dbn", G.DBN_CASES)):
        for name in cases:
            tiles, last = tile_count(fam, name)
            if "persist" in name:
                assert tiles > buffers(fam, name) * 256 and tiles % 256, (fam, name, tiles)
                assert fam not in G.PARTIAL_ROWS or tiles <= 3 * 256, (fam, name, tiles)
            else:
                assert 1 < tiles < 256, (fam, name, tiles)
            if "ragged" in name:
                assert last, (fam, name)


def buffers(fam, name):
    """LDS buffers a workgroup cycles its tiles through: three windows in conv3x1_dbn_kernel, three (window, gradient tile)
    pairs in conv3x1_wgrad_pipe_kernel, two patches / windows everywhere else"""
    return 3 if (fam == "dbn" and "stream" not in name) or (fam == "wgrad31" and "pipe" in name) else 2


def _sweep():
    for dname, dt in G.DTYPES.items():
        for N in (1, 3, 40, 300):
            for T in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 64):
                for H, W in ((1, 2), (2, 2), (2, 4), (4, 4), (4, 8), (8, 8), (7, 8), (8, 7), (14, 8), (13, 20), (28, 28), (56, 56), (3, 150), (5, 56)):
                    yield dname, dt, N, T, H, W


def test_unreachable_instantiations_are_never_planned():
    """over a sweep of clips, maps, channel pairs and both dtypes no call is planned on an UNREACHABLE symbol, every symbol that
    is planned has a case, and the sweep itself reaches the whole family"""
    seen = set()
    for dname, dt, N, T, H, W in _sweep():
        e = _T[dname]
        seen |= sym_win64(N, T, H * W, dt, e) | sym_win144(N, T, H * W, dt, e) | sym_wgrad31(N, T, H * W, dt, e)
        seen |= sym_bn_bwd(N, T, H * W, dt, e) | sym_stream31(N, T, H * W, dt, e)
        if T == 1:
            seen |= sym_c64(N, H, W, dt, e) | sym_stem(N, 2 * H, W, dt, e)
            for Cin, Cout in ((64, 144), (144, 64), (128, 288), (288, 128), (64, 64), (144, 144)):
                seen |= sym_stream(N, H, W, Cin, Cout, dt, e)
            for Cout in (48, 64, 80, 96, 128, 144, 160, 208, 288):
                seen |= sym_wgrad33(N, H, W, Cout, dt, e)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))
    assert seen <= set(WINDOW_COVERAGE), sorted(seen - set(WINDOW_COVERAGE))
    assert seen == set(WINDOW_COVERAGE), sorted(set(WINDOW_COVERAGE) - seen)


def test_plan_queries_refuse_what_the_launchers_refuse():
    from dvt_amd import ops
    lib, L = _lib()
    B = G.BF
    assert ops.conv3x1_c64_plan(3, 5, 32, B) is None and ops.conv3x1_c64_plan(3, 4, 32, torch.float32) is None
    assert ops.conv3x1_wgrad_plan(3, 5, 32, B) is None and not lib.dvt_conv3x1_wgrad_supported(3, 5, 32, 144, 64, L.BF16)
    assert ops.conv3x1_stream_bn_bwd_plan(2, 2, 32, B) is None and not lib.dvt_conv3x1_stream_supported(2, 2, 32, 64, 144, L.BF16)
    assert ops.conv3x3_c64_wgrad_plan(2, 13, 20, 60, B) is None and ops.conv3x3_c64_wgrad_plan(2, 13, 20, 72, B) is None
    assert ops.conv3x3_stream_plan(2, 13, 20, 64, 64, B) is None and ops.conv3x3_stream_plan(2, 13, 1, 64, 144, B) is None
    # the dtype picks the symbol, not the plan; the launches of a wide weight gradient tile the channels
    for Cout in (64, 80, 144, 160, 208, 288):
        for H, W in ((13, 20), (3, 150), (56, 56)):
            p = ops.conv3x3_c64_wgrad_plan(2, H, W, Cout, B)
            assert p == ops.conv3x3_c64_wgrad_plan(2, H, W, Cout, G.FP)
            assert p[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(p, p[1:])) and p[-1][0] + p[-1][1] == Cout
            assert all(mb == (5 if cv > 64 else 4 if cv > 16 else 1) and cv <= 16 * mb for _, cv, mb in p)
    # outputs are validated before anything else
    assert lib.dvt_conv3x1_c64_plan(3, 4, 32, L.BF16, None) == -1 and b"npb" in lib.dvt_last_error()
    assert lib.dvt_conv3x1_wgrad_plan(3, 4, 32, 144, 64, L.BF16, None) == -1
    assert lib.dvt_conv3x1_stream_bn_bwd_plan(3, 4, 64, L.BF16, None, None) == -1
    assert lib.dvt_conv3x3_stream_plan(2, 13, 20, 64, 144, L.BF16, None, None, None) == -1
    assert lib.dvt_conv3x3_c64_wgrad_plan(2, 13, 20, 64, L.BF16, 1, None, None, None, None) == -1


# ---------------------------------------------------------------- the tiles of a case (written out here; checked against the
# library's partial-row / workspace counts, which are one row (or 8, or 7: one per compute wave) per workgroup = per tile below 256 tiles)
def tile_rows(fam, name):
    """-> (rows of the map per tile R, or pixels per segment S for the window kernels)"""
    if fam == "c64":
        N, H, W = G.C64_CASES[name]
        return min(256 // W, H)
    if fam == "stream":
        (_, _, N, H, W), _ = G.STREAM_CASES[name]
        return min(224 // W, H)
    if fam == "stem":
        N, H, Wp = G.STEM_CASES[name]
        return min(896 // Wp, H // 2)
    if fam == "stream31":
        return {"ragged_5x112": 2, "persist_5x32": 5}[name]              # frames per tile (segments of 112 / 32 pixels)
    if fam == "wgrad33":                                                 # (the first, 64-wide launch; the plan query's)
        from dvt_amd import ops
        (N, H, W, Cout), _ = G.WGRAD33_CASES[name]
        return ops.conv3x3_c64_wgrad_plan(N, H, W, Cout, G.BF, rows=True)[0][3]
    if fam == "wgrad31":
        return 16 if "pipe" in name else 2                               # S: the map of the plain cases has 2 pixels per frame
    return 16                                                            # win64, dbn: segments of 16 pixels


def tile_count(fam, name):
    """-> (tiles of the launch, whether the last tile of an image is shorter than the others), checked against the library"""
    lib, L = _lib()
    r = tile_rows(fam, name)
    if fam == "c64":
        N, H, W = G.C64_CASES[name]
        tiles, parts = N * -(-H // r), lib.dvt_conv3x3_c64_stats_parts(N, H, W) // 8
    elif fam == "stream":
        (Cin, Cout, N, H, W), _ = G.STREAM_CASES[name]
        tiles, parts = N * -(-H // r), lib.dvt_conv3x3_stream_stats_parts(N, H, W, Cin, Cout) // 7
    elif fam == "stem":
        N, H, Wp = G.STEM_CASES[name]
        H = H // 2
        tiles, parts = N * -(-H // r), lib.dvt_conv_stem7_stats_parts(N, 2 * H, Wp)
    elif fam == "stream31":
        N, H, h, w = G.STREAM31_CASES[name]
        seg = {"ragged_5x112": 112, "persist_5x32": 32}[name]
        tiles, parts = N * (h * w // seg) * -(-H // r), None
    elif fam == "wgrad33":
        (N, H, W, Cout), _ = G.WGRAD33_CASES[name]
        tiles, parts = N * -(-H // r), lib.dvt_conv3x3_c64_wgrad_workspace_bytes(N, H, W) // (576 * 80 * 4)
    else:
        (N, H, h, w), _ = {"win64": G.WIN64_CASES, "wgrad31": G.WGRAD31_CASES, "dbn": G.DBN_CASES}[fam][name]
        if fam == "dbn" and "stream" in name:
            return tile_count("stream31", {"stream_ragged": "ragged_5x112", "stream_persist": "persist_5x32"}[name])
        tiles = N * (h * w // r)
        parts = (lib.dvt_conv3x1_fwd_stats_parts(N, H, h * w, 64) if fam == "win64" else
                 lib.dvt_conv3x1_wgrad_workspace_bytes(N, H, h * w) // (432 * 64 * 4) if fam == "wgrad31" else None)
        return _checked(tiles, parts, fam, name), False
    return _checked(tiles, parts, fam, name), H % r != 0


def _checked(tiles, parts, fam, name):
    if parts is not None:
        assert parts == min(tiles, 256), f"{fam} {name}: {tiles} tiles written out here, the library has {parts} workgroups"
    return tiles


# ---------------------------------------------------------------- bounds on the CPU
FWD = [("c64", n) for n in G.C64_CASES] + [("stream", n) for n in G.STREAM_CASES] + [("stream31", n) for n in G.STREAM31_CASES] + \
      [("win64", n) for n in G.WIN64_CASES] + [("stem", n) for n in G.STEM_CASES] + [("dbn", n) for n in G.DBN_CASES]
_BUILD = {"c64": G.build_c64, "stream": G.build_stream, "stream31": G.build_stream31, "win64": G.build_win64, "stem": G.build_stem,
          "dbn": G.build_dbn, "wgrad33": G.build_wgrad33, "wgrad31": G.build_wgrad31}
WG = [("wgrad33", n) for n in G.WGRAD33_CASES] + [("wgrad31", n) for n in G.WGRAD31_CASES]


def _integers(t):
    return torch.equal(t, t.round())


@pytest.mark.parametrize("fam,name", FWD, ids=[f"{f}-{n}" for f, n in FWD])
def test_forward_references_are_exact_in_both_types(fam, name):
    b = _BUILD[fam](name)
    if fam == "dbn":
        refs = [b["d"], b["dzm"], b["dz_eval"], b["dz_eval_norelu"]]
        assert _integers(b["d"]) and _integers(b["z"]) and _integers(b["dgamma"]) and _integers(b["dbeta"])
        for t in (b["dzm"] * b["z"], b["d"] * b["z"], b["d"]):
            assert float(t.abs().sum(0).max()) < 2 ** 24          # dgamma / dbeta exact under any summation order
        assert 0.3 < float(b["mask"].double().mean()) < 0.7       # the ReLU mask cuts roughly half
        assert bool(((b["gamma"].log2() % 1) == 0).all()) and _integers(b["beta"])
    else:
        refs = [b["y"]] + ([b["y"] + b["res"]] if "res" in b else []) + ([b["dx"]] if "dx" in b else [])
        assert all(_integers(t) for t in refs)
        if fam in G.PARTIAL_ROWS:
            G.check_partial_bound(b["y"], fam)
            if fam == "c64":
                G.check_partial_bound(b["y"] + b["res"], fam)
            assert float(V.stats_ref(b["y"].abs()).max()) < 2 ** 53      # (the float64 sum over the partial rows)
    for t in refs:
        for dt in G.DTYPES.values():
            X.check_bound(t, dt)


@pytest.mark.parametrize("fam,name", WG, ids=[f"{f}-{n}" for f, n in WG])
def test_wgrad_references_are_exact_in_fp32(fam, name):
    b = _BUILD[fam](name)
    assert _integers(b["dW"]) and _integers(b["prior"]) and float(b["dW"].abs().max()) + 4 < 2 ** 24
    assert float(V.wgrad_ref(b["x"], b["dz"].abs(), b["k"], 1, b["pad"]).max()) + 4 < 2 ** 24      # the sum of the magnitudes
    for dt in G.DTYPES.values():
        X.check_bound(b["x"], dt)
        X.check_bound(b["dz"], dt)


# ---------------------------------------------------------------- the operands see the faults
def _steps(k, ranges, tap_group):
    """-> [(taps of the k-step, lo, hi)]: one tap (the stem: one filter row) x one channel range"""
    kh, kw = V.pair(k)
    groups = {}
    for ki in range(kh):
        for kj in range(kw):
            groups.setdefault(ki * kw + kj if tap_group is None else tap_group(ki, kj), []).append((ki, kj))
    return [(taps, lo, hi) for _, taps in sorted(groups.items()) for lo, hi in ranges]


@pytest.mark.parametrize("fam,name", FWD, ids=[f"{f}-{n}" for f, n in FWD])
def test_forward_operands_see_the_faults(fam, name):
    """dropping or doubling any k-step changes every output some tap of which reads inside the map, and no other (so a border
    tap dropped at one border pixel shows in that pixel's row); a gather one pixel off in h / t or w, two swapped 16-byte
    channel slots of the pixels, a tile computed from the previous tile's patch and a shifted 16 x 16 output fragment change
    the reference in most of the elements they touch"""
    b = _BUILD[fam](name)
    pairs = [(b["dy"], b["wd"], b["d"], b["ranges"])] if fam == "dbn" else [(b["x"], b["w"], b["y"], b["ranges"])]
    if fam == "win64":
        pairs.append((b["dz"], b["wd"], b["dx"], G.R64))                # the data gradient as the convolution the kernel runs
        assert torch.equal(V.conv_ref(b["dz"], b["wd"], 1, (1, 0)), b["dx"])
    if fam == "dbn":
        assert torch.equal(V.dgrad_ref(b["dy"], b["wg"], b["geom"][2], b["geom"][3], 1, (1, 0)), b["d"])
    N, C, H, W, Cout, k, stride, pad = b["geom"]
    trim = b.get("trim_w", 0)
    for x, w, y, ranges in pairs:
        live = w.abs().sum((1, 2, 3)) > 0                              # output planes that exist (the data gradient's 45 of 64)
        nlive = int(live.sum())
        tap_total, tap_inb = {}, {}
        for taps, lo, hi in _steps(k, ranges, b["tap_group"]):
            part, inb = 0, torch.zeros(y.shape[0], dtype=torch.bool)
            for ki, kj in taps:
                p1, i1 = V.tap_range_partial(x, w, stride, pad, ki, kj, lo, hi, trim)
                part, inb = part + p1, inb | i1
                tap_total[(ki, kj)] = tap_total.get((ki, kj), 0) + p1
                tap_inb[(ki, kj)] = i1
            assert bool((part[inb][:, live] != 0).all()), f"k-step {taps} x [{lo}, {hi}) adds nothing to some in-bounds output"
            assert bool((part[~inb] == 0).all()) and bool((part[:, ~live] == 0).all()), f"k-step {taps} adds to an output it is padded at"
        some_padded = torch.zeros(y.shape[0], dtype=torch.bool)
        for i1 in tap_inb.values():
            some_padded |= ~i1
        assert bool(some_padded.any())
        for t, tot in tap_total.items():
            rows = some_padded & tap_inb[t]
            if bool(rows.any()):
                changed = (tot[rows] != 0).sum(1)
                assert int(changed.min()) >= nlive // 2, f"dropping tap {t} at a border pixel changes only {int(changed.min())} of {nlive} columns"
        for dh, dw in ((1, 0), (0, 1)):                                 # the gathered pixel one off (dh: a row, or a frame)
            off = V.conv_ref(V.shifted_map(x, dh, dw), w, stride, pad, trim)
            assert bool((off != y).any(1).all()), f"a gather shifted by ({dh}, {dw}) leaves some output rows unchanged"
            assert int((off != y)[:, live].sum()) * 2 >= y.shape[0] * nlive
        if C >= 16:                                                     # two 16-byte slots (8 channels each) of every pixel swapped
            s0 = 4 if C >= 48 else 0
            xs = x.clone()
            xs[..., 8 * s0:8 * s0 + 8], xs[..., 8 * s0 + 8:8 * s0 + 16] = x[..., 8 * s0 + 8:8 * s0 + 16], x[..., 8 * s0:8 * s0 + 8]
            sw = V.conv_ref(xs, w, stride, pad, trim)
            assert int((sw != y)[:, live].sum()) * 2 >= y.shape[0] * nlive, "swapping two channel slots changes under half of the outputs"
        # a tile computed from another tile's patch / window: the same tile of the previous image, the previous tile of this one
        yi = y.view(N, -1, Cout)[:, :, live]
        assert int((yi[1:] != yi[:-1]).sum()) * 2 >= yi[1:].numel()
        step = tile_rows(fam, name)
        if fam in ("win64", "dbn") and "stream" not in name:
            yt = y.view(N, H, W, Cout)[..., live]                       # segments of `step` pixels over all frames
            assert W > step and int((yt[:, :, step:] != yt[:, :, :-step]).sum()) * 2 >= yt[:, :, step:].numel()
        elif fam in ("c64", "stream", "stem") and "ragged" in name:
            Ho, Wo = V.out_hw(H, W, k, stride, pad, trim)
            yt = y.view(N, Ho, Wo, Cout)
            assert Ho > step and int((yt[:, step:] != yt[:, :-step]).sum()) * 2 >= yt[:, step:].numel()
        if "persist" in name:                                           # a stale LDS buffer: tile i comes out as tile i - 256
            segs = W // step if fam in ("win64", "dbn") and "stream" not in name else 1
            Ho, Wo = V.out_hw(H, W, k, stride, pad, trim)
            assert tile_count(fam, name)[0] == N * segs                 # (one tile per image / clip, or per segment of a clip)
            yt = y.view(N, Ho, segs, Wo // segs, Cout).permute(0, 2, 1, 3, 4).reshape(N * segs, -1, Cout)[..., live]
            assert int((yt[256:] != yt[:-256]).sum()) * 2 >= yt[256:].numel(), "tiles 256 apart share most of their outputs"
        for i in sorted({0, y.shape[0] // 32, y.shape[0] // 16 - 2}):    # a 16 x 16 output fragment taken from its neighbour
            for j in range(0, nlive // 16 - 1):
                for di, dj in ((1, 0), (0, 1)):
                    dchg = int((X.shifted_fragment(y, i, j, di, dj) != y).sum())
                    assert dchg >= 128, f"shifting fragment ({i}, {j}) by ({di}, {dj}) changes only {dchg} of 256 outputs"


def _wgrad_launches(fam, name):
    """-> [(first dz column, columns, [[rows of the flat pixel axis per 32-position step] per tile])] per launch, the tiles of
    the first and the last image / clip; the 3 x 3 kernel's rows per tile are the plan query's (an 80-wide group has its own)"""
    from dvt_amd import ops
    if fam == "wgrad33":
        (N, H, W, Cout), _ = G.WGRAD33_CASES[name]
        PW, out = W + 2, []
        for c0, cv, mb, R in ops.conv3x3_c64_wgrad_plan(N, H, W, Cout, G.BF, rows=True):
            tiles = []
            for n in (0, N - 1):
                for h0 in range(0, H, R):
                    rows = min(R, H - h0)
                    pos = {r * PW + c: (n * H + h0 + r) * W + c for r in range(rows) for c in range(W)}   # patch coordinates
                    tiles.append([[pos[p] for p in range(s, s + 32) if p in pos] for s in range(0, rows * PW, 32)])
            out.append((c0, cv, tiles))
        return out
    (N, T, H, W), _ = G.WGRAD31_CASES[name]
    Lp, S, tiles = H * W, tile_rows(fam, name), []
    for n in (0, N - 1):
        for sg in range(Lp // S):
            pos = [(n * T + t) * Lp + sg * S + sx for t in range(T) for sx in range(S)]
            tiles.append([pos[s:s + 32] for s in range(0, len(pos), 32)])
    return [(0, 64, tiles)]


@pytest.mark.parametrize("fam,name", WG, ids=[f"{f}-{n}" for f, n in WG])
def test_wgrad_operands_see_every_tile_and_position_step(fam, name):
    """per launch (the 80-wide group of the 3 x 3 kernel in its own tiling): dropping one tile, or one 32-position step of a
    tile, changes most of the entries of the launch's columns.  dz has one nonzero per column and 16 pixels of the flat pixel
    axis, so a step changes most entries once it holds 16 real pixels; only the LAST step of a 3 x 3 tile can hold fewer (k: the
    rest of the patch-row walk): such a step is seen through the columns whose nonzero lies inside it (about k / 16 of them),
    in most of their entries, and through no other column; the short steps are counted.  Shifting the gathered map by a pixel, or a 16 x 16 fragment of the gradient, changes
    most of what it touches."""
    b = _BUILD[fam](name)
    Cout = b["dz"].shape[-1]
    col = V.im2col(b["x"], b["k"], 1, b["pad"])
    dz = b["dz"].reshape(-1, Cout)
    full = col.t() @ dz
    kh, kw = V.pair(b["k"])
    assert torch.equal(full, b["dW"].permute(2, 3, 1, 0).reshape(kh * kw * b["x"].shape[-1], Cout))
    launches = _wgrad_launches(fam, name)
    assert [(c0, cv) for c0, cv, _ in launches] == ([(c0, cv) for c0, cv, _ in G.WGRAD33_CASES[name][1]] if fam == "wgrad33" else [(0, 64)])
    short = seen = 0
    for c0, cv, tiles in launches:
        for t in tiles:
            rows = torch.tensor([r for s in t for r in s])
            part = col[rows].t() @ dz[rows, c0:c0 + cv]
            assert int((part != 0).sum()) * 2 >= part.numel(), "dropping a tile changes under half of the gradient"
            for i, s in enumerate(t):
                k = len(s)
                assert k > 0
                part = col[torch.tensor(s)].t() @ dz[torch.tensor(s), c0:c0 + cv]
                if k >= 16:
                    assert int((part != 0).sum()) * 2 >= part.numel(), f"dropping positions {s[0]} .. {s[-1]} changes under half of the gradient"
                else:
                    assert fam == "wgrad33" and i == len(t) - 1, "a short position step that is not the last of its tile"
                    short += 1
                    hit = (dz[torch.tensor(s), c0:c0 + cv] != 0).any(0)
                    assert bool((part[:, ~hit] == 0).all())
                    if bool(hit.any()):
                        assert int((part[:, hit] != 0).sum()) * 2 >= part[:, hit].numel(), f"dropping the last {k} positions of a tile changes too little"
                    seen += int(hit.sum())
    assert short <= sum(len(tiles) for _, _, tiles in launches) and (short == 0 or seen > 0)
    for dh, dw in ((1, 0), (0, 1)):
        off = V.im2col(V.shifted_map(b["x"], dh, dw), b["k"], 1, b["pad"]).t() @ dz
        assert int((off != full).sum()) * 2 >= full.numel()
    for i in (0, full.shape[0] // 16 - 2):
        for j in range(0, Cout // 16 - 1, 2):
            for di, dj in ((1, 0), (0, 1)):
                assert int((X.shifted_fragment(full, i, j, di, dj) != full).sum()) >= 128
