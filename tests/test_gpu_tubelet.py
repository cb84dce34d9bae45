"""Tubelet embedding on the GPU (csrc/patchify.hip, ops.tubelet_patchify*, functional._PatchEmbed, ViViT(tubelet_size=),
AttentionRollout on a tubelet model) against the CPU restatement tests/tubelet_ref.py.

The gather is a permutation (plus one rounding to the destination type): bit-exact.  Embedding, model and rollout are held
to the project's per-operator bounds (tests/test_gpu_ops.py): rel-L2 <= 1e-4 in fp32, <= 1e-2 in
bf16 / fp16, against float64 ``conv3d`` autograd on the same dtype-rounded inputs, or -- the model under central
inflation -- against the per-frame path on the central frames, which the reference goldens pin."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import tubelet_ref as R
from tests.util import fill_state_from_numpy, rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
LP_TOL = 1e-2
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _tol(dtype):
    return F32_TOL if dtype == torch.float32 else LP_TOL


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


# ---------------------------------------------------------------- the gather
GPU_SHAPES = R.GATHER_SHAPES + [
    (2, 8, 3, 64, 64, 16, 2),      # 128 rows, more than one wave per workgroup
    (1, 4, 3, 32, 32, 16, 1),      # pt = 1: must equal ops.patchify
]
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("f16", "f16"), ("f32", "f16"), ("bf16", "f32"), ("f16", "f32")]


@functools.lru_cache(maxsize=None)
def _clip_and_ref(shape, src):
    """(clip in the source type, its gather as fp32) -- computed once per (shape, source type), never written to."""
    b, t, C, H, W, P, pt = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(b, t, C, H, W, generator=g).to(DT[src])
    return x, R.gather(x.float(), P, pt)


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_bit_exact(dvt, device, shape, pair):
    b, t, C, H, W, P, pt = shape
    src, dst = pair
    x, ref = _clip_and_ref(shape, src)
    out = dvt.ops.tubelet_patchify(x.to(device), P, pt, DT[dst])
    assert out.dtype == DT[dst] and out.shape == ref.shape
    assert torch.equal(out.cpu(), ref.to(DT[dst]))
    if pt == 1:
        assert torch.equal(out, dvt.ops.patchify(x.to(device), P, DT[dst]))


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_adjoint_is_the_inverse(dvt, device, shape):
    b, t, C, H, W, P, pt = shape
    x, ref = _clip_and_ref(shape, "f32")
    out = dvt.ops.tubelet_patchify(x.to(device), P, pt, torch.float32)
    back = dvt.ops.tubelet_patchify_bwd(out, x.shape, P, pt, torch.float32)
    assert back.shape == x.shape and torch.equal(back.cpu(), x)
    # a bf16 dout into an f32 dx
    xb, _ = _clip_and_ref(shape, "bf16")
    dout = dvt.ops.tubelet_patchify(xb.to(device), P, pt, torch.bfloat16)
    back = dvt.ops.tubelet_patchify_bwd(dout, xb.shape, P, pt, torch.float32)
    assert back.dtype == torch.float32 and torch.equal(back.cpu(), xb.float())
    # and against the restatement directly: the scatter of an arbitrary dout
    g = torch.Generator().manual_seed(3)
    d = torch.randn(ref.shape, generator=g)
    dx = dvt.ops.tubelet_patchify_bwd(d.to(device), x.shape, P, pt, torch.float32).cpu()
    assert torch.equal(R.gather(dx, P, pt), d)


def test_ops_refuse_what_is_not_whole_tubelets(dvt, device):
    x = torch.zeros(2, 3, 3, 16, 16, device=device)
    with pytest.raises(ValueError, match="tubelets"):
        dvt.ops.tubelet_patchify(x, 8, 2, torch.float32)
    with pytest.raises(ValueError, match="tubelet"):
        dvt.ops.tubelet_patchify(x, 8, 0, torch.float32)
    with pytest.raises(RuntimeError, match="dvt_tubelet_patchify"):
        dvt.ops.tubelet_patchify(torch.zeros(1, 2, 3, 20, 16, device=device), 8, 2, torch.float32)


# ---------------------------------------------------------------- F.patch_embed(..., tubelet=2)
@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
def test_patch_embed_tubelet_fwd_bwd(dvt, device, tag):
    F = dvt.functional
    dtype = DT[tag]
    b, t, C, H, W, P, pt, d = 2, 4, 3, 32, 32, 8, 2, 64
    K = pt * P * P * C
    g = torch.Generator().manual_seed(17)
    clip = torch.randn(b, t, C, H, W, generator=g).to(dtype).float()          # dtype-rounded values, fp32 storage
    w = (torch.randn(d, K, generator=g) / K ** 0.5).to(dtype).float()
    bias = 0.1 * torch.randn(d, generator=g)
    rows = b * (t // pt) * (H // P) * (W // P)
    dy = torch.randn(rows, d, generator=g).to(dtype)
    # float64 conv3d autograd on the same values
    c64, w64, b64 = (v.double().requires_grad_() for v in (clip, w, bias))
    ref = R.embed_conv3d(c64, w64, b64, P, pt)
    ref.backward(dy.double())
    cd, wd, bd = (v.to(device).requires_grad_() for v in (clip, w, bias))
    emb = F.patch_embed(cd, wd, bd, P, dtype, tubelet=pt)
    assert emb.shape == (rows, d) and emb.dtype == dtype
    emb.backward(dy.to(device))
    errs = {"emb": rel_l2(emb, ref), "dW": rel_l2(wd.grad, w64.grad), "db": rel_l2(bd.grad, b64.grad),
            "dclip": rel_l2(cd.grad, c64.grad)}
    print(f"[tubelet] patch_embed {tag}: {errs}")
    assert cd.grad.shape == clip.shape and cd.grad.dtype == torch.float32
    assert all(v <= _tol(dtype) for v in errs.values()), errs
    # a clip without a gradient gets none, and the parameters' gradients are the same
    w2, b2 = (v.to(device).requires_grad_() for v in (w, bias))
    F.patch_embed(clip.to(device), w2, b2, P, dtype, tubelet=pt).backward(dy.to(device))
    assert torch.equal(w2.grad, wd.grad) and torch.equal(b2.grad, bd.grad)


# ---------------------------------------------------------------- the model under central inflation
CFG = dict(dim=64, depth=2, heads=2, dim_head=32)


def _models(dvt, dtype, device):
    """(tubelet model loaded from a per-frame checkpoint, the per-frame model of the central frames)."""
    from dvt_amd.models.vit import ViViT
    src = ViViT(32, 8, 19, 4, compute_dtype=dtype, **CFG)
    fill_state_from_numpy(src.named_parameters(), 2024)
    tub = ViViT(32, 8, 19, 4, compute_dtype=dtype, tubelet_size=2, **CFG)
    tub.load_frame_checkpoint(src.state_dict(), mode="central")
    ref = ViViT(32, 8, 19, 2, compute_dtype=dtype, **CFG)
    sd = dict(src.state_dict())
    sd["pos_embedding"] = sd["pos_embedding"][:, 1::2].clone()
    ref.load_state_dict(sd)
    return tub.to(device), ref.to(device)


def _clip(device):
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.standard_normal((2, 4, 3, 32, 32)).astype(np.float32)).to(torch.bfloat16).float()
    y = torch.from_numpy((rng.random((2, 19)) < 0.3).astype(np.float32))
    return x.to(device), y.to(device)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_model_under_central_inflation_is_the_per_frame_model_of_the_central_frames(dvt, device, tag, monkeypatch):
    F = dvt.functional
    dtype = DT[tag]
    tol = _tol(dtype)
    tub, ref = _models(dvt, dtype, device)
    x, y = _clip(device)
    xc = x[:, 1::2].contiguous()
    tub.eval(), ref.eval()
    with torch.no_grad():
        e = rel_l2(tub(x), ref(xc))
    print(f"[tubelet] model {tag}: forward logits rel {e:.2e}")
    assert e <= tol
    # loss + backward; the gradient at the embedding is kept for the float64 reference of the patch weight's gradient
    kept = {}
    plain = F.patch_embed

    def tapped(*a, **k):
        emb = plain(*a, **k)
        if k.get("tubelet", 1) != 1:
            emb.register_hook(lambda gr: kept.__setitem__("demb", gr.detach().clone()))
        return emb

    monkeypatch.setattr(F, "patch_embed", tapped)
    tub.train(), ref.train()
    loss_t, logits_t = tub.loss(x, y)
    loss_t.backward()
    loss_r, logits_r = ref.loss(xc, y)
    loss_r.backward()
    errs = {"logits": rel_l2(logits_t, logits_r)}
    gt, gr = dict(tub.named_parameters()), dict(ref.named_parameters())
    assert list(gt) == list(gr)
    pw = "to_patch_embedding.1.weight"
    for k in gt:
        if k != pw:
            assert gt[k].grad.shape == gr[k].grad.shape, k
            errs[k] = rel_l2(gt[k].grad, gr[k].grad)
    blocks = gt[pw].grad.reshape(64, 2, 192)
    errs[pw + "[central]"] = rel_l2(blocks[:, 1], gr[pw].grad)
    # the off-central block: float64 conv3d autograd from the model's own embedding gradient
    demb = kept["demb"].double().cpu()
    w64 = gt[pw].detach().double().cpu().requires_grad_()
    xin = x.cpu().to(dtype).double()
    R.embed_conv3d(xin, w64, None, 8, 2).backward(demb)
    ref_blocks = w64.grad.reshape(64, 2, 192)
    errs[pw + "[off-central]"] = rel_l2(blocks[:, 0], ref_blocks[:, 0])
    assert float(ref_blocks[:, 0].norm()) > 0.1 * float(ref_blocks[:, 1].norm())   # a zero weight block still learns
    worst = max(errs, key=errs.get)
    print(f"[tubelet] model {tag}: loss {float(loss_t.detach()):.5f} / {float(loss_r.detach()):.5f}; worst {worst} {errs[worst]:.2e}")
    assert all(v <= tol for v in errs.values()), {k: v for k, v in errs.items() if v > tol}


# ---------------------------------------------------------------- rollout
def test_rollout_on_a_tubelet_model(dvt, device):
    from dvt_amd.rollout import AttentionRollout
    tub, ref = _models(dvt, torch.float32, device)
    x, _ = _clip(device)
    ro_t, ro_r = AttentionRollout(tub), AttentionRollout(ref)
    space, time, video = ro_t.maps(x)
    assert space.shape == video.shape == (2, 2, 4, 4) and time.shape == (2, 2)
    mask = ro_t(x)
    assert mask.shape == (2, 4, 32, 32) and mask.dtype == torch.float32
    assert float(mask.min()) >= 0.0 and float(mask.max()) <= 1.0
    assert ro_t(x, size=(2, 16, 16)).shape == (2, 2, 16, 16)
    # the per-frame model keeps its default: the clip's own (t, H, W)
    xc = x[:, 1::2].contiguous()
    assert ro_r(xc).shape == (2, 2, 32, 32)
    errs = {n: rel_l2(a, b) for n, a, b in zip(("space", "time", "video"), (space, time, video), ro_r.maps(xc))}
    print(f"[tubelet] rollout maps against the per-frame model of the central frames: {errs}")
    assert all(v <= F32_TOL for v in errs.values()), errs
