"""Mixup / CutMix without a GPU: the host draws of dvt_amd.input_stage.Mixup (timm's rule), its Beta sampler against
scipy, the float64 restatement tests/mix_ref.py against torch, and the C surface of csrc/mix.hip (declarations, host-side
validation of every argument before any HIP call)."""
import ctypes
import math
import os
import re

import pytest
import torch

from dvt_amd.input_stage import Mixup, draw_beta, scale_box      # the feature: a tree without it fails here, at import
from tests import mix_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dvt_clips_mix", "dvt_targets_mix", "dvt_ce_soft_fwd", "dvt_ce_soft_bwd")


def _mixup(**kw):
    kw.setdefault("generator", torch.Generator().manual_seed(7))
    return Mixup(**kw)


# ---------------------------------------------------------------- the draws
@pytest.mark.parametrize("box", ["tube", "spatiotemporal", "temporal"])
@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_draw_rules(mode, box):
    T, H, W = 6, 17, 23
    m = _mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, box=box)
    kinds = set()
    for B in (1, 4, 5, 8) * 6:
        table, lam_in, lam_t = m.draw(B, T, H, W)
        assert table.shape == (B, 8) and table.dtype == torch.int32
        assert lam_in.shape == (B,) and lam_t.shape == (B,) and lam_in.dtype == lam_t.dtype == torch.float32
        assert table[:, 0].tolist() == list(range(B - 1, -1, -1))                       # the partner is the flip
        for i, (p, kind, t0, t1, y0, y1, x0, x1) in enumerate(table.tolist()):
            kinds.add(kind)
            assert kind in (0, 1, 2) and 0.0 <= float(lam_in[i]) <= 1.0 and 0.0 <= float(lam_t[i]) <= 1.0
            if kind == 2:
                assert 0 <= t0 <= t1 <= T and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W     # inside the clip
                vol = (t1 - t0) * (y1 - y0) * (x1 - x0)
                assert float(lam_t[i]) == float(torch.tensor(1.0 - vol / (T * H * W), dtype=torch.float32))
                if box == "tube":
                    assert (t0, t1) == (0, T)
                if box == "temporal":
                    assert (y0, y1, x0, x1) == (0, H, 0, W)
            elif kind == 1:
                assert float(lam_t[i]) == float(lam_in[i])
            else:
                assert float(lam_t[i]) == 1.0 and float(lam_in[i]) == 1.0
        rows = [tuple(r[1:]) + (float(a), float(b)) for r, a, b in zip(table.tolist(), lam_in, lam_t)]
        if mode == "batch":
            assert len(set(rows)) == 1
        if mode == "pair":
            assert rows == rows[::-1]                                                   # mirrored onto both members
            if B % 2:
                assert rows[B // 2][0] == 0                                             # the middle sample is left alone
    assert kinds >= {1, 2}
    if mode == "elem":
        table, lam_in, _ = m.draw(16, T, H, W)
        assert len({tuple(r[1:]) + (float(a),) for r, a in zip(table.tolist(), lam_in)}) > 8                         # one draw per sample


def test_prob_zero_and_seed():
    table, lam_in, lam_t = _mixup(prob=0.0, cutmix_alpha=1.0, mode="elem").draw(6, 4, 8, 8)
    assert table[:, 1].tolist() == [0] * 6 and lam_in.tolist() == [1.0] * 6 and lam_t.tolist() == [1.0] * 6
    a = _mixup(cutmix_alpha=1.0, mode="elem", generator=torch.Generator().manual_seed(3)).draw(9, 4, 20, 30)
    b = _mixup(cutmix_alpha=1.0, mode="elem", generator=torch.Generator().manual_seed(3)).draw(9, 4, 20, 30)
    c = _mixup(cutmix_alpha=1.0, mode="elem", generator=torch.Generator().manual_seed(4)).draw(9, 4, 20, 30)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[0], c[0])
    only_cut = _mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem").draw(12, 4, 20, 30)[0]
    assert set(only_cut[:, 1].tolist()) <= {0, 2}
    only_mix = _mixup(mixup_alpha=1.0, cutmix_alpha=0.0, mode="elem").draw(12, 4, 20, 30)[0]
    assert set(only_mix[:, 1].tolist()) <= {0, 1}


def test_box_side_rule():
    """timm's rand_bbox: sides int(size * sqrt(1 - lam)) before clipping, so an unclipped box has exactly those sides"""
    from dvt_amd import input_stage as S
    g = torch.Generator().manual_seed(11)
    for _ in range(50):
        lo, hi = S._cut(40, 0.5, g)
        assert 0 <= lo <= hi <= 40 and hi - lo <= 20
        if lo > 0 and hi < 40:
            assert hi - lo == 20
    assert scale_box([0, 13, 3, 9, 2, 5], (13, 224, 224), (156, 112, 112)) == [0, 156, 1, 5, 1, 3]
    assert scale_box([0, 13, 0, 224, 7, 7], (13, 224, 224), (156, 112, 112)) == [0, 156, 0, 112, 3, 3]


def test_beta_sampler_against_scipy():
    """4096 draws of Beta(0.8, 0.8) at seed 0: the Kolmogorov-Smirnov statistic is below the 0.1 %-level critical value"""
    from scipy import stats
    n = 4096
    x = draw_beta(0.8, torch.Generator().manual_seed(0), n=n).numpy()
    assert x.shape == (n,) and (x >= 0).all() and (x <= 1).all()
    d = stats.kstest(x, stats.beta(0.8, 0.8).cdf).statistic
    assert d < 1.95 / math.sqrt(n), d
    assert isinstance(draw_beta(0.8, torch.Generator().manual_seed(0)), float)


def test_surface_refusals():
    from dvt_amd import ops
    with pytest.raises(NotImplementedError, match="cutmix_minmax"):
        Mixup(cutmix_minmax=(0.2, 0.8))
    with pytest.raises(ValueError, match="mode"):
        Mixup(mode="half")
    with pytest.raises(ValueError, match="num_classes"):
        Mixup()(torch.zeros(2, 1, 3, 4, 4), torch.zeros(2, dtype=torch.int64))
    x = torch.zeros(3, 2, 3, 4, 4)
    lam = [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match=r"\[rows, 8\]"):
        ops.clips_mix(x, [(0, 0, 0, 0)] * 3, lam)
    with pytest.raises(ValueError, match="table rows"):
        ops.clips_mix(x, [(0, 0, 0, 0, 0, 0, 0, 0)] * 2, lam)
    with pytest.raises(ValueError, match="lam"):
        ops.clips_mix(x, [(0, 0, 0, 0, 0, 0, 0, 0)] * 3, [1.0])
    with pytest.raises(ValueError, match="contiguous"):
        ops.clips_mix(x.transpose(3, 4), [(0, 0, 0, 0, 0, 0, 0, 0)] * 3, lam)
    with pytest.raises(ValueError, match="involution"):
        ops.clips_mix(x, [(1, 1, 0, 0, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0)], lam)
    with pytest.raises(ValueError, match=r"\[rows, 8\]"):
        ops.targets_mix([(0, 0)] * 3, lam, y=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="exactly one"):
        ops.targets_mix([(0,) * 8] * 3, lam)
    with pytest.raises(ValueError, match="num_classes"):
        ops.targets_mix([(0,) * 8] * 3, lam, labels=torch.zeros(3, dtype=torch.int64))


# ---------------------------------------------------------------- the restatement
def test_reference_statements():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 2, 3, 5, 6, generator=g, dtype=torch.float64)
    lam = [0.25, 1.0, 0.5, 0.75]
    table = [(3, 1, 0, 0, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0, 0, 0), (1, 2, 1, 2, 1, 4, 2, 5), (0, 0, 0, 2, 0, 5, 0, 6)]
    out = MR.clips_mix(x, table, lam)
    assert torch.equal(out[0], 0.25 * x[0] + 0.75 * x[3]) and torch.equal(out[1], x[1]) and torch.equal(out[3], x[3])
    want = x[2].clone()
    want[1:2, :, 1:4, 2:5] = x[1, 1:2, :, 1:4, 2:5]
    assert torch.equal(out[2], want)
    labels = torch.tensor([1, 0, 6, 3])
    rows = MR.label_rows(labels, 7, 0.1, torch.float64)
    import torch.nn.functional as TF
    logits = torch.randn(4, 7, generator=g, dtype=torch.float64)
    loss, lse, tsum = MR.ce_soft(logits, rows)
    assert abs(float(loss) - float(TF.cross_entropy(logits, labels, label_smoothing=0.1))) < 1e-7
    assert torch.allclose(tsum, torch.ones(4, dtype=torch.float64), atol=1e-6)
    soft = 2.0 * torch.softmax(torch.randn(4, 7, generator=g, dtype=torch.float64), 1)         # rows that sum to 2
    lr = logits.clone().requires_grad_(True)
    l2, lse2, ts2 = MR.ce_soft(lr, soft)
    (gx,) = torch.autograd.grad(l2, lr, torch.tensor(1.7, dtype=torch.float64))
    assert torch.allclose(MR.ce_soft_bwd(logits, soft, lse2, ts2, torch.tensor(1.7, dtype=torch.float64)), gx, atol=1e-12)
    mixed = MR.targets_mix(rows, table, lam)
    assert torch.equal(mixed[1], rows[1]) and torch.allclose(mixed[0], 0.25 * rows[0] + 0.75 * rows[3])
    assert torch.isnan(MR.label_rows(torch.tensor([7, 0]), 7, 0.0, torch.float64)[0]).all()


# ---------------------------------------------------------------- C surface
def _lib():
    import dvt_amd
    return dvt_amd._lib.load()


def test_header_declares_the_entry_points():
    import dvt_amd
    header = open(os.path.join(ROOT, "include", "dvt_hip.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", header) and n in dvt_amd._lib.SIGNATURES and hasattr(_lib(), n)
    assert "SoftTargetCrossEntropy" in header and "basicmlp.py:38" in header and "MMX_Frame_dl.py:63-88" in header
    assert _lib().dvt_version() == 5 and dvt_amd._lib.ABI_VERSION == 5
    assert dvt_amd.ops.MIX_ROWS_PER_LAUNCH == dvt_amd._lib.MACROS["DVT_MIX_ROWS_PER_LAUNCH"] >= 1


def _i32(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def _f32(vals):
    return (ctypes.c_float * len(vals))(*vals)


def _clips(lib, rows, lam, out=None, x=64, B=None, T=4, H=8, W=12):
    """dvt_clips_mix on dummy non-null device pointers: everything is validated before anything touches them"""
    tab, lm = _i32(rows), _f32(lam)
    return lib.dvt_clips_mix(x, out, 1, len(rows) if B is None else B, T, 3, H, W, ctypes.cast(tab, ctypes.c_void_p),
                             ctypes.cast(lm, ctypes.c_void_p), None)




def _rows(bad):
    """four rows, partner = flip, the bad one at index 2"""
    return [(3, 1, 0, 0, 0, 0, 0, 0), (2, 2, 1, 3, 2, 5, 3, 9), bad, (0, 0, 9, 9, 9, 9, 9, 9)]


def test_null_pointers_are_refused_by_name():
    lib = _lib()
    p = 64
    one = ctypes.cast(_i32([(0,) * 8]), ctypes.c_void_p)
    lam = ctypes.cast(_f32([1.0]), ctypes.c_void_p)
    for args in ((None, None, 0, 1, 1, 3, 4, 4, one, lam, None), (p, None, 0, 1, 1, 3, 4, 4, None, lam, None),
                 (p, None, 0, 1, 1, 3, 4, 4, one, None, None)):
        assert lib.dvt_clips_mix(*args) == -1 and b"dvt_clips_mix" in lib.dvt_last_error()
    for args in ((p, None, None, 1, 4, one, lam, 0.0, None), (p, None, p, 1, 4, None, lam, 0.0, None),
                 (p, None, p, 1, 4, one, None, 0.0, None), (None, None, p, 1, 4, one, lam, 0.0, None),
                 (p, p, p, 1, 4, one, lam, 0.0, None)):
        assert lib.dvt_targets_mix(*args) == -1 and b"dvt_targets_mix" in lib.dvt_last_error()
    for args in ((None, 4, p, p, p, 3, 4, 0, None), (p, 4, None, p, p, 3, 4, 0, None), (p, 4, p, None, p, 3, 4, 0, None),
                 (p, 4, p, p, None, 3, 4, 0, None), (p, 3, p, p, p, 3, 4, 0, None), (p, 4, p, p, p, 0, 4, 0, None),
                 (p, 4, p, p, p, 3, 4, 7, None)):
        assert lib.dvt_ce_soft_fwd(*args) == -1 and b"dvt_ce_soft_fwd" in lib.dvt_last_error()
    for args in ((None, 4, p, p, p, p, 4, 3, 4, 0, None), (p, 4, None, p, p, p, 4, 3, 4, 0, None),
                 (p, 4, p, None, p, p, 4, 3, 4, 0, None), (p, 4, p, p, None, p, 4, 3, 4, 0, None),
                 (p, 4, p, p, p, None, 4, 3, 4, 0, None), (p, 4, p, p, p, p, 3, 3, 4, 0, None)):
        assert lib.dvt_ce_soft_bwd(*args) == -1 and b"dvt_ce_soft_bwd" in lib.dvt_last_error()


@pytest.mark.parametrize("bad,what", [((1, 2, 0, 5, 0, 8, 0, 12), b"leaves"), ((1, 2, 0, 4, 0, 8, 7, 6), b"leaves"),
                                      ((1, 2, 0, 4, -1, 8, 0, 12), b"leaves"), ((1, 2, 0, 4, 0, 9, 0, 12), b"leaves"),
                                      ((1, 2, 0, 4, 0, 8, 0, 13), b"leaves"), ((1, 2, 3, 2, 0, 8, 0, 12), b"leaves"),
                                      ((4, 1, 0, 0, 0, 0, 0, 0), b"partner"), ((-1, 1, 0, 0, 0, 0, 0, 0), b"partner"),
                                      ((1, 3, 0, 0, 0, 0, 0, 0), b"kind"), ((1, -1, 0, 0, 0, 0, 0, 0), b"kind")])
def test_bad_clip_row_is_named(bad, what):
    lib = _lib()
    assert _clips(lib, _rows(bad), [0.5, 0.5, 0.5, 1.0]) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_clips_mix" in msg and b"row 2" in msg and what in msg, msg


@pytest.mark.parametrize("lam", [-0.25, 1.5, float("nan"), float("inf")])
def test_bad_lambda_is_named(lam):
    lib = _lib()
    assert _clips(lib, _rows((1, 1, 0, 0, 0, 0, 0, 0)), [0.5, 0.5, lam, 1.0]) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_clips_mix" in msg and b"row 2" in msg and b"lam" in msg, msg
    tab = ctypes.cast(_i32(_rows((1, 1, 0, 0, 0, 0, 0, 0))), ctypes.c_void_p)
    assert lib.dvt_targets_mix(64, None, 64, 4, 7, tab, ctypes.cast(_f32([0.5, 0.5, lam, 1.0]), ctypes.c_void_p), 0.0, None) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_targets_mix" in msg and b"row 2" in msg and b"lam" in msg, msg


def test_partner_map_rules():
    lib = _lib()
    roll = [(1, 1, 0, 0, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0)]
    lam = [0.5] * 4
    for out in (None, 64):                                   # out == NULL and out == x are both in place
        assert _clips(lib, roll, lam, out=out) == -1
        msg = lib.dvt_last_error()
        assert b"dvt_clips_mix" in msg and b"row 0" in msg and b"involution" in msg, msg
    nbytes = 4 * 4 * 3 * 8 * 12 * 2
    assert _clips(lib, roll, lam, out=64 + nbytes - 2) == -1 and b"overlaps" in lib.dvt_last_error()
    assert _clips(lib, roll, lam, x=65) == -1 and b"aligned" in lib.dvt_last_error()
    tab = ctypes.cast(_i32(roll), ctypes.c_void_p)
    lm = ctypes.cast(_f32(lam), ctypes.c_void_p)
    assert lib.dvt_clips_mix(64, None, 7, 4, 4, 3, 8, 12, tab, lm, None) == -1 and b"dtype" in lib.dvt_last_error()
    assert lib.dvt_clips_mix(64, None, 0, 4, 4, 0, 8, 12, tab, lm, None) == -1 and b"shape" in lib.dvt_last_error()
    assert lib.dvt_clips_mix(64, None, 0, 4, 1 << 14, 1, 1 << 8, 1 << 8, tab, lm, None) == -1 and b"2^30" in lib.dvt_last_error()
    bad = ctypes.cast(_i32([(0,) * 8, (4,) + (0,) * 7, (2,) + (0,) * 7, (3,) + (0,) * 7]), ctypes.c_void_p)
    assert lib.dvt_targets_mix(64, None, 64, 4, 7, bad, lm, 0.0, None) == -1
    assert b"row 1" in lib.dvt_last_error() and b"partner" in lib.dvt_last_error()
    assert lib.dvt_targets_mix(64, None, 64, 4, 7, tab, lm, 1.0, None) == -1 and b"smoothing" in lib.dvt_last_error()
