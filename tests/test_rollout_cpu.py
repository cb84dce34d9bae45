"""Attention rollout without a GPU: the float64 restatement against the reference fixture, the fixture's own fitness, the
host-only plan query, the argument checks of the C ABI and the refusals of the public class."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rollout_ref as R
from tests.util import golden


@pytest.fixture(scope="module")
def fx():
    g = golden("attention_rollout.npz")
    return {k: g[k] for k in g.files}


def _qkv(fx):
    return [torch.from_numpy(a) for a in fx["qkv_space"]], [torch.from_numpy(a) for a in fx["qkv_time"]]


def test_restatement_reproduces_the_fixture(fx):
    sp, tm = _qkv(fx)
    r_space, r_time, video = R.vivit_rollout(sp, tm, int(fx["cfg_heads"]), float(fx["rho"]))
    for got, name in ((r_space, "r_space"), (r_time, "r_time"), (video, "video")):
        assert got.dtype == torch.float64
        assert float((got - torch.from_numpy(fx[name])).abs().max()) <= 1e-12, name


def test_rows_sum_to_one(fx):
    for name in ("r_space", "r_time"):
        assert np.abs(fx[name].sum(1) - 1.0).max() <= 1e-12, name
    sp, tm = R.vivit_layers(*_qkv(fx), int(fx["cfg_heads"]))
    Rm = R.rollout_matrix(sp, float(fx["rho"]))
    assert float((Rm.sum(-1) - 1.0).abs().max()) <= 1e-12
    # the uniform start (mean pooling) keeps the total as well
    assert float((R.rollout(tm, float(fx["rho"]), query=None).sum(1) - 1.0).abs().max()) <= 1e-12


def test_fixture_can_tell_a_wrong_kernel(fx):
    """(a) peaked maps, (b) a rotated key order moves the answer, (c) the exponent range the kernel bound is derived for."""
    sp, tm = _qkv(fx)
    ratio, diff, smax = R.fixture_conditions(torch.from_numpy(fx["r_space"]), sp, tm, int(fx["cfg_heads"]), float(fx["rho"]))
    assert ratio >= 5.0
    assert diff >= 0.1
    assert smax <= 20.0
    for tag in ("bf16", "fp16"):
        for name in ("r_space", "r_time", "video"):
            assert 0.0 < float(fx[f"{tag}:{name}_err"]) < 0.1


def test_restatement_is_oriented_as_the_definition():
    """r0^T Ahat with a permutation matrix P (query i attends to key perm[i]): the mass of token i moves TO perm[i]."""
    N, rho = 5, 0.25
    perm = torch.tensor([1, 2, 3, 4, 0])
    q = torch.zeros(1, 1, N, N, dtype=torch.float64)
    k = torch.zeros(1, 1, N, N, dtype=torch.float64)
    for i in range(N):
        q[0, 0, i, i] = 1.0
    for j in range(N):
        k[0, 0, j] = -200.0
    for i in range(N):
        k[0, 0, perm[i], i] = 0.0
    r0 = torch.tensor([[0.5, 0.25, 0.125, 0.0625, 0.0625]], dtype=torch.float64)
    got = R.step(q, k, 1.0, r0, rho)
    want = rho * r0
    for i in range(N):
        want[0, perm[i]] += (1 - rho) * r0[0, i]
    assert float((got - want).abs().max()) <= 1e-15


# ---------------------------------------------------------------- the C ABI without a device
def _views(S, H, N, dh, dtype, Lq=None):
    Lq = N if Lq is None else Lq
    qkv = torch.zeros(S, N, 3, H, dh, dtype=dtype)
    q = qkv[:, :Lq, 0].permute(0, 2, 1, 3)
    k = qkv[:, :, 1].permute(0, 2, 1, 3)
    return q, k


def test_plan_answers_without_a_device():
    from dvt_amd import ops
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    assert ops.ROLLOUT_FORMS == ("none", "mfma", "generic")
    r = torch.zeros(2, 197)
    p = ops.rollout_plan(*_views(2, 8, 197, 64, bf), r)
    assert p.form == "mfma" and p.key_steps == 7 and p.query_parts == 2 and p.waves == 14 and 0 < p.lds <= 160 * 1024
    for N, steps in ((16, 1), (17, 1), (33, 2), (325, 11), (352, 11), (353, 12), (512, 16)):
        for dtype in (bf, hf):
            p = ops.rollout_plan(*_views(1, 2, N, 64, dtype), torch.zeros(1, N))
            assert p.form == "mfma" and p.key_steps == steps and p.waves == steps * p.query_parts <= 16, (N, p)
            assert p.lds <= 160 * 1024
    # the uniform start is dense as well; a one-hot start is one query row: the generic form
    assert ops.rollout_plan(*_views(2, 8, 33, 64, bf), None, query=ops.ROLLOUT_UNIFORM).form == "mfma"
    assert ops.rollout_plan(*_views(2, 8, 197, 64, bf), None, query=0).form == "generic"
    assert ops.rollout_plan(*_views(2, 8, 197, 64, bf, Lq=1), None, query=0).form == "generic"
    # past the MFMA form's length, other head dims, fp32: generic
    assert ops.rollout_plan(*_views(1, 1, 513, 64, bf), torch.zeros(1, 513)).form == "generic"
    assert ops.rollout_plan(*_views(2, 2, 14, 448, bf), torch.zeros(2, 14)).form == "generic"
    assert ops.rollout_plan(*_views(2, 2, 14, 448, f32), torch.zeros(2, 14)).form == "generic"
    assert ops.rollout_plan(*_views(3, 4, 5, 32, f32), torch.zeros(3, 5)).form == "generic"
    assert ops.rollout_plan(*_views(2, 2, 17, 64, f32), torch.zeros(2, 17)).form == "generic"
    assert ops.rollout_plan(*_views(0, 2, 17, 64, bf), torch.zeros(0, 17)).form == "none"
    # what the launcher refuses: more than the LDS holds
    with pytest.raises(RuntimeError, match="LDS budget"):
        ops.rollout_plan(*_views(1, 1, 30000, 64, f32), torch.zeros(1, 30000))
    # ... and what the wrapper refuses before it gets there
    with pytest.raises(ValueError, match="query"):
        ops.rollout_plan(*_views(1, 1, 17, 64, bf), None, query=17)
    with pytest.raises(ValueError, match="one-hot"):
        ops.rollout_plan(*_views(1, 1, 17, 64, bf, Lq=1), torch.zeros(1, 17))
    with pytest.raises(ValueError, match="residual"):
        ops.rollout_plan(*_views(1, 1, 17, 64, bf), torch.zeros(1, 17), residual=1.5)
    with pytest.raises(TypeError):
        ops.rollout_plan(torch.zeros(1, 1, 17, 64), torch.zeros(1, 1, 16, 32), None)


def test_null_and_bad_arguments_fail_before_any_hip_call():
    from dvt_amd import _lib
    lib = _lib.load()
    assert lib.dvt_version() == 5
    info = _lib.RolloutPlanInfo()
    assert lib.dvt_rollout_step(None, None) == -1 and b"dvt_rollout_step" in lib.dvt_last_error()
    assert lib.dvt_rollout_plan(None, C.byref(info)) == -1 and b"dvt_rollout_plan" in lib.dvt_last_error()
    d = _lib.RolloutDesc()
    assert lib.dvt_rollout_plan(C.byref(d), None) == -1 and b"dvt_rollout_plan" in lib.dvt_last_error()
    assert lib.dvt_rollout_from_probs(None, 1, 17, 2, 0, 0.5, None, None) == -1
    assert b"dvt_rollout_from_probs" in lib.dvt_last_error()
    assert lib.dvt_rollout_from_probs(None, 1, 17, 9, 0, 0.5, None, None) == -1            # more heads than P carries
    assert lib.dvt_rollout_video(None, None, 1, 3, 16, None, None, None) == -1
    assert b"dvt_rollout_video" in lib.dvt_last_error()
    # a descriptor with data pointers missing, Lq that is neither N nor 1, a stored r_in with one query row
    d.S, d.H, d.N, d.Lq, d.dh, d.dtype, d.rho, d.scale = 1, 1, 17, 17, 64, _lib.BF16, 0.5, 0.125
    assert lib.dvt_rollout_step(C.byref(d), None) == -1 and b"null q" in lib.dvt_last_error()
    d.Lq = 3
    assert lib.dvt_rollout_step(C.byref(d), None) == -1 and b"Lq" in lib.dvt_last_error()
    d.Lq, d.r_in = 1, 256
    assert lib.dvt_rollout_step(C.byref(d), None) == -1 and b"one-hot" in lib.dvt_last_error()
    # empty batches launch nothing and need no device
    assert lib.dvt_rollout_from_probs(None, 0, 17, 2, 0, 0.5, None, None) == 0
    assert lib.dvt_rollout_video(None, None, 0, 3, 16, None, None, None) == 0


def test_ops_need_the_gpu():
    from dvt_amd import ops
    q, k = _views(1, 1, 17, 64, torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_step(q, k, torch.zeros(1, 1, 17), torch.zeros(1, 17))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_from_probs(torch.zeros(1, 17, 8), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_video(torch.zeros(3, 17), torch.zeros(1, 4))


def test_unsupported_models_are_refused():
    from dvt_amd.rollout import AttentionRollout
    from dvt_amd.models.vit import ViViT, Transformer
    from dvt_amd.models.frame_transformer import FrameTransformer
    with pytest.raises(NotImplementedError, match="ViViT"):
        AttentionRollout(Transformer(64, 1, 2, 32, 128))
    with pytest.raises(NotImplementedError, match="ViViT"):
        AttentionRollout(torch.nn.Linear(4, 4))
    enc = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="'vid'"):
        AttentionRollout(FrameTransformer(model="frame", d_model=64, nhead=2, nhid=64, nlayers=1, img_encoder=enc, vid_encoder=enc))
    with pytest.raises(ValueError, match="residual"):
        AttentionRollout(ViViT(32, 8, 5, 3, dim=64, depth=1, heads=2, dim_head=32), residual=2.0)
    ro = AttentionRollout(ViViT(32, 8, 5, 3, dim=64, depth=1, heads=2, dim_head=32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ro.maps(torch.zeros(1, 3, 3, 32, 32))


def test_tap_is_off_by_default_and_restored_when_the_body_raises():
    from dvt_amd import functional as F
    assert F._attn_tap is None
    with pytest.raises(KeyError):
        with F.attention_tap() as layers:
            assert F._attn_tap is layers == []
            with F.attention_tap() as inner:
                assert F._attn_tap is inner
            assert F._attn_tap is layers
            raise KeyError("x")
    assert F._attn_tap is None
