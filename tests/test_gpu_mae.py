"""Masked-autoencoder pre-training on the GPU (csrc/mae.hip, ops.tokens_restore_* / mae_loss_*, functional.tokens_restore /
mae_loss, models.mae.MaskedClipAutoencoder) against the float64 CPU statement tests/mae_ref.py and the reference golden
tests/golden/mae.npz.

The restore is one fp32 select and add with one rounding: bit-equal to torch's.  Its backward on small-integer gradients, and
the loss on small integers with power-of-two divisors: exact.  Everything else is held to the project's per-operator bounds
(tests/test_gpu_patch_dropout.py): rel-L2 <= 1e-4 for fp32 outputs of fp32 arithmetic, <= 1e-2 for
outputs rounded to 16 bits, against the restatement on the same dtype-rounded inputs; the fp32 model against the golden of the
imported reference modules.  No test here feeds an out-of-range index."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import mae_ref as M
from tests import patchdrop_ref as PR
from tests import tubelet_ref as TR
from tests.util import fill_state_from_numpy, golden, rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
LP_TOL = 1e-2
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FENCE = 64                                         # elements on either side of a raw output buffer
UNTRAINED = ("encoder.temporal_transformer.", "encoder.temporal_token", "encoder.mlp_head.")


def _tol(dtype):
    return F32_TOL if dtype == torch.float32 else LP_TOL


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fenced(numel, dtype, fill, fence_value, device):
    """A buffer of ``numel`` elements filled with ``fill`` between two fences of FENCE elements -> (whole, the middle view)."""
    whole = torch.full((numel + 2 * FENCE,), fence_value, dtype=dtype, device=device)
    mid = whole[FENCE:FENCE + numel]
    mid.fill_(fill)
    return whole, mid


def _fences_intact(whole, fence_value):
    return bool((whole[:FENCE] == fence_value).all()) and bool((whole[-FENCE:] == fence_value).all())


def _keep_slot(S, n, k, seed):
    keys = torch.from_numpy(np.random.default_rng(seed).integers(0, 100000, (S, n))).to(torch.int32)
    return PR.keep_select(keys, k)


# ---------------------------------------------------------------- restore
RESTORE_SHAPES = [(8, 4, 16, 5, 32, 1), (6, 3, 196, 20, 384, 1), (4, 4, 9, 1, 40, 1), (4, 2, 100, 100, 48, 0)]  # S T n k d skip


@functools.lru_cache(maxsize=None)
def _restore_case(shape, tag):
    """(y, mask, pos, keep, slot, integer dout, float dout) on the CPU in the dtype ``tag``; never written."""
    S, T, n, k, d, skip = shape
    g = torch.Generator().manual_seed(sum(shape))
    y = torch.randn(S, skip + k, d, generator=g).to(DT[tag])
    mask, pos = torch.randn(d, generator=g), torch.randn(T, n, d, generator=g)
    keep, slot = _keep_slot(S, n, k, sum(shape) + 1)
    dint = torch.randint(-4, 5, (S, n, d), generator=g).to(DT[tag])
    dflt = torch.randn(S, n, d, generator=g).to(DT[tag])
    return y, mask, pos, keep, slot, dint, dflt


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", RESTORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restore_forward_bit_equal(dvt, device, shape, tag):
    ops = dvt.ops
    S, T, n, k, d, skip = shape
    y, mask, pos, keep, slot, _, _ = _restore_case(shape, tag)
    # torch's fp32 where and add, rounded once
    rows = y.float().gather(1, (slot.long().clamp(min=0) + skip)[:, :, None].expand(S, n, d))
    ref = (torch.where((slot >= 0)[:, :, None], rows, mask.expand(S, n, d)) + pos[torch.arange(S) % T]).to(DT[tag])
    assert bool((slot < 0).any()) == (k < n)
    yd, md, pd_, sd = y.to(device), mask.to(device), pos.to(device), slot.to(device)
    out = ops.tokens_restore_fwd(yd, md, pd_, sd, k, skip)
    assert out.shape == (S, n, d) and out.dtype == DT[tag]
    assert torch.equal(out.cpu(), ref)
    # straight through the C entry into a NaN-filled, fenced buffer: every row written, nothing around it
    whole, mid = _fenced(S * n * d, DT[tag], float("nan"), 77.0, device)
    lib = dvt._lib.load()
    dvt._lib.check(lib.dvt_tokens_restore_fwd(yd.data_ptr(), md.data_ptr(), pd_.data_ptr(), sd.data_ptr(), mid.data_ptr(), S, T,
                                              n, k, skip, d, ops.dt(yd), _stream()))
    torch.cuda.synchronize()
    assert _fences_intact(whole, 77.0) and torch.equal(mid.view(S, n, d), out)


def test_restore_refuses_a_width_that_is_no_multiple_of_8(dvt, device, monkeypatch):
    launched = []
    lib = dvt._lib.load()
    monkeypatch.setattr(dvt._lib, "load", lambda: launched.append(1) or lib)
    slot = torch.zeros(4, 16, dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="multiple of 8"):
        dvt.ops.tokens_restore_fwd(torch.zeros(4, 6, 36, device=device), torch.zeros(36, device=device),
                                   torch.zeros(2, 16, 36, device=device), slot, 5)
    with pytest.raises(ValueError, match="multiple of 8"):
        dvt.ops.tokens_restore_bwd(torch.zeros(4, 16, 36, device=device), slot[:, :5].contiguous(), slot, 2)
    assert not launched                                           # refused before the library was even asked


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RESTORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restore_backward_exact_and_deterministic(dvt, device, shape, tag):
    ops = dvt.ops
    S, T, n, k, d, skip = shape
    _, _, _, keep, slot, dint, dflt = _restore_case(shape, tag)
    kd, sd = keep.to(device), slot.to(device)
    rdy, rdmask, rdpos = M.restore_adjoint(dint.double(), keep, slot, T, skip)
    # through the C entry: fenced outputs, NaN-filled -- every element written once, nothing around them
    lib = dvt._lib.load()
    dd = dint.to(device)
    wy, dy = _fenced(S * (skip + k) * d, DT[tag], float("nan"), 77.0, device)
    wm, dmask = _fenced(d, torch.float32, float("nan"), 77.0, device)
    wp, dpos = _fenced(T * n * d, torch.float32, float("nan"), 77.0, device)
    wq, part = _fenced(T * n * d, torch.float32, float("nan"), 77.0, device)
    dvt._lib.check(lib.dvt_tokens_restore_bwd(dd.data_ptr(), kd.data_ptr(), sd.data_ptr(), dy.data_ptr(), dmask.data_ptr(),
                                              dpos.data_ptr(), part.data_ptr(), S, T, n, k, skip, d, ops.dt(dd), 0, _stream()))
    torch.cuda.synchronize()
    assert all(_fences_intact(w, 77.0) for w in (wy, wm, wp, wq))
    assert torch.equal(dy.cpu().double().view(S, skip + k, d), rdy)                 # a permutation of rows of dout
    assert torch.equal(dmask.cpu().double(), rdmask) and torch.equal(dpos.cpu().double().view(T, n, d), rdpos)
    if skip:
        assert bool((dy.view(S, skip + k, d)[:, :skip] == 0).all())
    if k == n:
        assert bool((dmask == 0).all()) and not bool(torch.signbit(dmask).any())
    # the wrapper; accumulate adds onto a prefilled sink, overwrite ignores it
    acc_m, acc_p = torch.full((d,), 1.5, device=device), torch.full((T, n, d), 3.25, device=device)
    dy2, m2, p2 = ops.tokens_restore_bwd(dd, kd, sd, T, skip, dmask=acc_m, dpos=acc_p, accumulate=True)
    assert m2 is acc_m and p2 is acc_p and torch.equal(dy2.view(-1), dy)
    assert torch.equal(acc_m.cpu().double(), 1.5 + rdmask) and torch.equal(acc_p.cpu().double(), 3.25 + rdpos)
    ops.tokens_restore_bwd(dd, kd, sd, T, skip, dmask=acc_m, dpos=acc_p, accumulate=False)
    assert torch.equal(acc_m.cpu().double(), rdmask) and torch.equal(acc_p.cpu().double(), rdpos)
    # random floats: two runs bit-equal, and the restatement within the per-operator bound
    df = dflt.to(device)
    a, b = ops.tokens_restore_bwd(df, kd, sd, T, skip), ops.tokens_restore_bwd(df, kd, sd, T, skip)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    ref = M.restore_adjoint(dflt.double(), keep, slot, T, skip)
    errs = {name: rel_l2(u, v) for name, u, v in zip(("dy", "dmask", "dpos"), a, ref)}
    print(f"[mae] restore backward {tag} {shape}: {errs}")
    assert errs["dy"] == 0.0 and errs["dpos"] <= F32_TOL
    assert errs["dmask"] <= F32_TOL or k == n


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_functional_restore_against_float64_autograd(dvt, device, tag):
    F = dvt.functional
    shape = RESTORE_SHAPES[0]
    S, T, n, k, d, skip = shape
    y, mask, pos, keep, slot, _, dflt = _restore_case(shape, tag)
    leaves = [v.double().requires_grad_() for v in (y, mask, pos)]
    ref = M.restore(*leaves, slot, skip)
    ref.backward(dflt.double())
    yd = y.to(device).requires_grad_()
    md, pd_ = mask.view(1, 1, d).to(device).requires_grad_(), pos.view(1, T, n, d).to(device).requires_grad_()
    out = F.tokens_restore(yd, md, pd_, keep.to(device), slot.to(device), S, T, skip=skip)
    out.backward(dflt.to(device))
    assert md.grad.shape == (1, 1, d) and pd_.grad.shape == (1, T, n, d) and yd.grad.shape == y.shape
    errs = {"out": rel_l2(out, ref), "dy": rel_l2(yd.grad, leaves[0].grad), "dmask": rel_l2(md.grad, leaves[1].grad),
            "dpos": rel_l2(pd_.grad, leaves[2].grad)}
    assert all(v <= _tol(DT[tag]) for v in errs.values()), errs


# ---------------------------------------------------------------- the loss
def _loss_both(dvt, device, pred, clip, slot, k, P, pt, norm_pix, seed=1.0):
    """(loss, per_patch, stats, dpred) of the two raw wrappers; per_patch into a fenced buffer through the C entry as well."""
    ops = dvt.ops
    pd_, cd, sd = pred.to(device), clip.to(device), slot.to(device)
    loss, per, stats = ops.mae_loss_fwd(pd_, cd, sd, k, P, pt, norm_pix)
    g = torch.full((1,), seed, device=device)
    dpred = ops.mae_loss_bwd(pd_, cd, sd, k, P, pt, stats, g)
    assert loss.dtype == per.dtype == torch.float32 and per.shape == slot.shape and dpred.dtype == pred.dtype
    assert (stats is None) == (not norm_pix)
    return loss, per, stats, dpred


def test_loss_exact_on_small_integers(dvt, device):
    """norm_pix off, C = 4, P = 4 (D = 64), b, t, pt = 2, 2, 1, a 16 x 16 image (n = 16), k = 8: M D = 2048.  Every sum stays
    below 2^24 and every divisor is a power of two: fp32 equals float64 bit for bit."""
    b, t, C, H, P, pt, k = 2, 2, 4, 16, 4, 1, 8
    S, n, D = b * t, 16, 64
    clip = TR.integer_clip((b, t, C, H, H), seed=5)
    pred = TR.integer_clip((S, n, D), seed=6)
    keep, slot = _keep_slot(S, n, k, 7)
    rl, rper = M.loss(pred, clip, slot, P, pt, False)
    rg = M.loss_grad(pred, clip, slot, P, pt, False)
    loss, per, _, dpred = _loss_both(dvt, device, pred.float(), clip.float(), slot, k, P, pt, False)
    assert torch.equal(per.cpu().double(), rper) and float(loss) == float(rl)
    assert torch.equal(dpred.cpu().double(), rg)
    kept = slot >= 0
    assert bool((per.cpu()[kept] == 0).all()) and bool((dpred.cpu()[kept] == 0).all()) and int(kept.sum()) == S * k
    assert bool((per.cpu()[~kept] > 0).all())
    # fenced outputs through the C entries: every element written, nothing around them
    ops, lib = dvt.ops, dvt._lib.load()
    pd_, cd, sd = pred.float().to(device), clip.float().to(device), slot.to(device)
    wper, fper = _fenced(S * n, torch.float32, float("nan"), 77.0, device)
    wl, fl = _fenced(1, torch.float32, float("nan"), 77.0, device)
    wd, fd = _fenced(S * n * D, torch.float32, float("nan"), 77.0, device)
    one = torch.ones(1, device=device)
    dvt._lib.check(lib.dvt_mae_loss_fwd(pd_.data_ptr(), ops.dt(pd_), cd.data_ptr(), ops.dt(cd), sd.data_ptr(), fper.data_ptr(),
                                        None, fl.data_ptr(), b * t, C, H, H, P, pt, k, 0, 1e-6, _stream()))
    dvt._lib.check(lib.dvt_mae_loss_bwd(pd_.data_ptr(), ops.dt(pd_), cd.data_ptr(), ops.dt(cd), sd.data_ptr(), None,
                                        one.data_ptr(), fd.data_ptr(), b * t, C, H, H, P, pt, k, 0, _stream()))
    torch.cuda.synchronize()
    assert all(_fences_intact(w, 77.0) for w in (wper, wl, wd))
    assert torch.equal(fper.view(S, n), per) and torch.equal(fl, loss) and torch.equal(fd.view(S, n, D), dpred)


def test_loss_upstream_gradient_is_a_device_scalar(dvt, device):
    """loss.backward(seed) with a device scalar 1024 gives exactly 1024 x the gradient of seed 1, on the exact case."""
    F = dvt.functional
    b, t, C, H, P, pt, k = 2, 2, 4, 16, 4, 1, 8
    clip = TR.integer_clip((b, t, C, H, H), seed=5).float().to(device)
    keep, slot = _keep_slot(b * t, 16, k, 7)
    grads = []
    for seed in (1.0, 1024.0):
        pred = TR.integer_clip((b * t, 16, 64), seed=6).float().to(device).requires_grad_()
        loss, per = F.mae_loss(pred, clip, slot.to(device), k, P, pt, norm_pix=False)
        assert loss.dim() == 0 and not per.requires_grad
        loss.backward(torch.full((), seed, device=device))
        grads.append(pred.grad)
    assert bool((grads[0] != 0).any()) and torch.equal(grads[1], grads[0] * 1024.0)
    assert torch.equal(grads[0].cpu().double(), M.loss_grad(TR.integer_clip((b * t, 16, 64), seed=6),
                                                            TR.integer_clip((b, t, C, H, H), seed=5), slot, P, pt, False))


LOSS_SHAPES = [(2, 4, 3, 32, 32, 8, 1, 5), (2, 4, 3, 32, 32, 8, 2, 5), (1, 2, 3, 224, 224, 16, 2, 20)]   # b t C H W P pt k
LOSS_TYPES = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32")]                          # pred, clip


@functools.lru_cache(maxsize=None)
def _loss_case(shape):
    b, t, C, H, W, P, pt, k = shape
    S, n, D = b * t // pt, (H // P) * (W // P), pt * P * P * C
    g = torch.Generator().manual_seed(sum(shape))
    clip = torch.randn(b, t, C, H, W, generator=g)
    pred = torch.randn(S, n, D, generator=g)
    keep, slot = _keep_slot(S, n, k, sum(shape) + 1)
    return clip, pred, slot


@functools.lru_cache(maxsize=None)
def _loss_ref(shape, ptag, ctag, norm_pix):
    clip, pred, slot = _loss_case(shape)
    P, pt = shape[5], shape[6]
    c64, p64 = clip.to(DT[ctag]).double(), pred.to(DT[ptag]).double()
    return M.loss(p64, c64, slot, P, pt, norm_pix) + (M.loss_grad(p64, c64, slot, P, pt, norm_pix),)


@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("types", LOSS_TYPES, ids=["-".join(p) for p in LOSS_TYPES])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_against_the_restatement(dvt, device, shape, types, norm_pix):
    ptag, ctag = types
    b, t, C, H, W, P, pt, k = shape
    clip, pred, slot = _loss_case(shape)
    rl, rper, rg = _loss_ref(shape, ptag, ctag, norm_pix)
    loss, per, stats, dpred = _loss_both(dvt, device, pred.to(DT[ptag]), clip.to(DT[ctag]), slot, k, P, pt, norm_pix)
    errs = {"loss": abs(float(loss) - float(rl)) / abs(float(rl)), "per_patch": rel_l2(per, rper), "dpred": rel_l2(dpred, rg)}
    print(f"[mae] loss {shape} pred {ptag} clip {ctag} norm_pix {norm_pix}: {errs}")
    kept = slot >= 0
    assert bool((per.cpu()[kept] == 0).all()) and bool((dpred.cpu()[kept] == 0).all())
    assert errs["loss"] <= F32_TOL and errs["per_patch"] <= F32_TOL and errs["dpred"] <= _tol(DT[ptag]), errs
    if norm_pix:
        full = M.targets(clip.to(DT[ctag]).double(), P, pt, False)
        assert rel_l2(stats.cpu()[..., 0][~kept], full.mean(-1)[~kept]) <= F32_TOL
        assert rel_l2(stats.cpu()[..., 1][~kept], (full.var(-1) + M.EPS).rsqrt()[~kept]) <= F32_TOL
        assert bool((stats.cpu()[kept] == 0).all())


def test_loss_refuses_a_clip_that_cannot_be_masked(dvt, device):
    with pytest.raises(ValueError, match="M == 0"):
        dvt.ops.mae_loss_fwd(torch.zeros(1, 1, 192, device=device), torch.zeros(1, 1, 3, 8, 8, device=device),
                             torch.zeros(1, 1, dtype=torch.int32, device=device), 1, 8, 1, True)
    with pytest.raises(ValueError, match="M == 0"):
        dvt.functional.mae_loss(torch.zeros(8, 16, 192, device=device), torch.zeros(2, 4, 3, 32, 32, device=device),
                                torch.zeros(8, 16, dtype=torch.int32, device=device), 16, 8, 1)


@pytest.mark.parametrize("shape", [LOSS_SHAPES[0], LOSS_SHAPES[2]], ids=["D192", "D1536"])
def test_loss_statistics_on_offset_patches(dvt, device, shape):
    """An fp32 clip of 100 + 0.5 N(0, 1): the variance as a sum of squared deviations from the mean keeps per_patch and dpred
    within 1e-4 (a float32 simulation measured 1.0e-5 .. 1.1e-5); E[x^2] - E[x]^2 would lose them (2.0e-3 .. 2.2e-3)."""
    b, t, C, H, W, P, pt, k = shape
    clip, pred, slot = _loss_case(shape)
    clip = (100.0 + 0.5 * clip).float()
    rl, rper = M.loss(pred.double(), clip.double(), slot, P, pt, True)
    rg = M.loss_grad(pred.double(), clip.double(), slot, P, pt, True)
    loss, per, _, dpred = _loss_both(dvt, device, pred, clip, slot, k, P, pt, True)
    errs = {"loss": abs(float(loss) - float(rl)) / abs(float(rl)), "per_patch": rel_l2(per, rper), "dpred": rel_l2(dpred, rg)}
    print(f"[mae] offset patches {shape}: {errs}")
    assert all(v <= F32_TOL for v in errs.values()), errs


def test_loss_on_constant_patches(dvt, device):
    """norm_pix on a constant patch: the variance is 0, the target 0; the loss and dpred are finite."""
    shape = LOSS_SHAPES[0]
    b, t, C, H, W, P, pt, k = shape
    _, pred, slot = _loss_case(shape)
    clip = torch.full((b, t, C, H, W), 3.0)
    loss, per, stats, dpred = _loss_both(dvt, device, pred, clip, slot, k, P, pt, True)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(per).all()) and bool(torch.isfinite(dpred).all())
    rl, rper = M.loss(pred.double(), clip.double(), slot, P, pt, True)
    assert bool((M.targets(clip.double(), P, pt, True) == 0).all())
    assert rel_l2(per, rper) <= F32_TOL and abs(float(loss) - float(rl)) <= F32_TOL * float(rl)
    assert rel_l2(dpred, M.loss_grad(pred.double(), clip.double(), slot, P, pt, True)) <= F32_TOL


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _golden():
    g = golden("mae.npz")
    return g, {k[4:]: int(g[k]) for k in g.files if k.startswith("cfg_")}


def _golden_net(dtype, device, tubelet=1, **kw):
    from dvt_amd.models import MaskedClipAutoencoder
    from dvt_amd.models.vit import ViViT
    g, cfg = _golden()
    enc = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"], compute_dtype=dtype, tubelet_size=tubelet)
    kw.setdefault("mask_ratio", 0.7)                   # k = 16 - floor(11.2) = 5, the fixture's
    net = MaskedClipAutoencoder(enc, decoder_dim=cfg["dec_dim"], decoder_depth=cfg["dec_depth"], decoder_heads=cfg["dec_heads"],
                                decoder_dim_head=cfg["dec_dim_head"], **kw)
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return net.to(device)


def _round_parameters_(net, dtype):
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(dtype).float())


def _golden_inputs():
    g, _ = _golden()
    return torch.from_numpy(g["clip"]), torch.from_numpy(g["keep"])


def _ref_kw(cfg, **kw):
    return dict(patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"], dec_depth=cfg["dec_depth"],
                dec_heads=cfg["dec_heads"], **kw)


def _check_step(tag, net, loss, ref_loss, ref_grads, tol, grad_scale=1.0):
    errs = {"loss": abs(float(loss.detach()) - float(ref_loss)) / abs(float(ref_loss))}
    params = dict(net.named_parameters())
    for name, p in params.items():
        if name.startswith(UNTRAINED):
            assert p.grad is None and name not in ref_grads, name
            continue
        assert p.grad is not None and p.grad.shape == ref_grads[name].shape, name
        errs[name] = rel_l2(p.grad / grad_scale, ref_grads[name])
    assert sorted(errs) == sorted(["loss"] + list(ref_grads))
    worst = max(errs, key=errs.get)
    print(f"[mae] model {tag}: loss {float(loss.detach()):.6f} / {float(ref_loss):.6f}; worst {worst} {errs[worst]:.2e}")
    assert all(v <= tol for v in errs.values()), {k_: v for k_, v in errs.items() if v > tol}


@pytest.mark.parametrize("norm", ["norm", "raw"])
def test_model_fp32_against_the_reference_golden(dvt, device, norm):
    g, cfg = _golden()
    clip, keep = _golden_inputs()
    net = _golden_net(torch.float32, device, norm_pix_loss=norm == "norm").train()
    loss, pred, slot = net(clip.to(device), keep=keep.to(device))
    loss.backward()
    assert pred.shape == (8, 16, 192) and torch.equal(slot.cpu(), PR.slots_of(keep, 16)) and net.last_keep.shape == (8, 5)
    ref_grads = {k[len(norm) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(norm + ":g:")}
    _check_step(f"fp32 / golden / {norm}", net, loss, float(g[norm + ":loss"]), ref_grads, F32_TOL)
    # the mask token's gradient comes from the dropped positions only, the positional table's from every position
    assert bool((net.decoder_pos_embedding.grad.abs().sum(-1) > 0).all())


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_model_16bit_against_the_restatement(dvt, device, tag):
    """fp16 runs under a loss scale of 1024 (a power of two: scaling and unscaling are exact), as the project trains in fp16:
    the loss gradient 2 / (M D) (pred - target) is ~1e-4 per element here, at the edge of fp16's normal range."""
    g, cfg = _golden()
    dtype = DT[tag]
    clip, keep = _golden_inputs()
    clip = clip.to(dtype).float()
    net = _golden_net(dtype, device).train()
    _round_parameters_(net, dtype)
    P = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    ref_loss, _, ref_grads = M.masked_step(clip.double(), P, keep, **_ref_kw(cfg))
    loss, _, _ = net(clip.to(device), keep=keep.to(device))
    scale = 1024.0 if dtype == torch.float16 else 1.0
    loss.backward(torch.full((), scale, device=device))
    _check_step(tag + " / restatement", net, loss, ref_loss, ref_grads, LP_TOL, grad_scale=scale)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_tubelet_model_against_the_restatement(dvt, device, tag):
    g, cfg = _golden()
    dtype = DT[tag]
    clip, keep = _golden_inputs()
    b = clip.shape[0]
    net = _golden_net(dtype, device, tubelet=2, norm_pix_loss=True).train()
    if dtype != torch.float32:
        _round_parameters_(net, dtype)
        clip = clip.to(dtype).float()
    keep2 = keep.reshape(b, cfg["frames"], -1)[:, 1::2].reshape(b * cfg["frames"] // 2, -1).contiguous()
    P = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    ref_loss, _, ref_grads = M.masked_step(clip.double(), P, keep2, pt=2, **_ref_kw(cfg))
    loss, pred, _ = net(clip.to(device), keep=keep2.to(device))
    loss.backward()
    assert pred.shape == (4, 16, 384)
    _check_step(tag + " / pt = 2", net, loss, ref_loss, ref_grads, _tol(dtype))


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("mode", ["tube", "frame"])
def test_drawing_tube_and_frame(dvt, device, mode, monkeypatch):
    F = dvt.functional
    F.manual_seed(5)                                    # a fixed draw; no captured graph is alive here
    clip, _ = _golden_inputs()
    x = clip.to(device)
    net = _golden_net(torch.float32, device, mask_ratio=0.5, mask_mode=mode).train()
    seen = []
    plain = dvt.ops.keep_draw

    def tapped(*a, **k):
        r = plain(*a, **k)
        seen.append((a, r))
        return r

    monkeypatch.setattr(dvt.ops, "keep_draw", tapped)
    site = F._rng.site
    loss, pred, slot = net(x)
    loss.backward()
    (args, (keep, slot_drawn)), = seen
    b, t, n = 2, 4, 16
    assert keep.shape == (b * t, 8) and keep.dtype == torch.int32 and net.last_keep is keep and slot is slot_drawn
    assert torch.equal(dvt.ops.keep_slots(keep, n), slot)
    rows = keep.cpu().view(b, t, 8)
    if mode == "tube":
        assert args[0] == b and bool((rows == rows[:, :1]).all()) and not torch.equal(rows[0, 0], rows[1, 0])
        assert F._rng.site - site == (b * n + 3) // 4
    else:
        assert args[0] == b * t and all(len({tuple(r) for r in clip_rows.tolist()}) > 1 for clip_rows in rows)
        assert F._rng.site - site == (b * t * n + 3) // 4
    # passing the drawn keep back reproduces the loss and the gradients bit for bit
    g1 = _grads(net)
    net.zero_grad(set_to_none=True)
    loss2, pred2, _ = net(x, keep=keep)
    loss2.backward()
    assert len(seen) == 1 and torch.equal(loss2, loss) and torch.equal(pred2, pred)
    g2 = _grads(net)
    assert sorted(g1) == sorted(g2) and all(torch.equal(v, g1[k]) for k, v in g2.items())
    # a masked autoencoder always masks: eval mode draws too
    net.eval()
    with torch.no_grad():
        le, _, _ = net(x)
    assert len(seen) == 2 and net.last_keep.shape == (b * t, 8) and bool(torch.isfinite(le))
    F.next_step()


# ---------------------------------------------------------------- FlatParameters: sinks and no_sync
def test_flat_parameters_sinks_and_no_sync(dvt, device):
    from dvt_amd.dp import FlatParameters
    clip, keep1 = _golden_inputs()
    x = clip.to(device)
    keep2, _ = _keep_slot(keep1.shape[0], 16, 7, 41)                                     # another subset, another k
    k1, k2 = keep1.to(device), keep2.to(device)
    plain = _golden_net(torch.float32, device).train()
    separate = []
    for kp in (k1, k2):
        plain.zero_grad(set_to_none=True)
        plain(x, keep=kp)[0].backward()
        separate.append(_grads(plain))
    net = _golden_net(torch.float32, device).train()
    flat = FlatParameters(net, compute_dtype=None)
    seed = torch.full((), flat.loss_scale, device=device)
    unused = [name for name, _ in net.named_parameters() if name.startswith(UNTRAINED)]
    assert len(unused) > 10
    # one step with sinks
    flat.zero_grad()
    net(x, keep=k1)[0].backward(seed)
    flat.finish_backward()
    params = dict(net.named_parameters())
    errs = {k: rel_l2(params[k].grad, v) for k, v in separate[0].items()}
    assert all(v <= F32_TOL for v in errs.values()), errs
    assert all(bool((params[k].grad == 0).all()) for k in unused)
    # a window of two micro-batches with different keeps: the sum of the two
    flat.zero_grad()
    with flat.no_sync():
        net(x, keep=k1)[0].backward(seed)
        flat.finish_backward()
    net(x, keep=k2)[0].backward(seed)
    flat.finish_backward()
    errs = {k: rel_l2(params[k].grad, v + separate[1][k]) for k, v in separate[0].items()}
    print(f"[mae] no_sync window of two keeps: worst {max(errs.values()):.2e}")
    assert all(v <= F32_TOL for v in errs.values()), errs
    assert all(bool((params[k].grad == 0).all()) for k in unused)


# ---------------------------------------------------------------- a captured step draws a new mask on every replay
def _training_run(dvt, device, steps, capture):
    """Seed once, build, then ``steps`` steps of zero_grad; loss; backward; finish_backward; next_step -- eagerly, or one
    warm-up step and replays of the captured step.  Everything the captured graph addresses stays referenced from this frame
    until after the last replay and a synchronize."""
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    F = dvt.functional
    F.manual_seed(77)                                   # before anything is built; never between capture and replay
    clip, _ = _golden_inputs()
    x = clip.to(device)
    net = _golden_net(torch.float32, device, mask_ratio=0.5).train()
    flat = FlatParameters(net, compute_dtype=None)
    seed = torch.full((), flat.loss_scale, device=device)
    state = F._rng.tensor(x.device)

    def step(net=net, flat=flat, seed=seed, x=x):
        flat.zero_grad()
        loss, _, _ = net(x)
        loss.backward(seed)
        flat.finish_backward()
        F.next_step()
        return loss

    losses = []
    if capture:
        replay, out = capture_step(step, warmup=1)
        for _ in range(steps - 1):
            replay()
            losses.append(float(out.detach()))
        torch.cuda.synchronize()
        assert F._rng.state is state                    # the generator state the graph addresses is still the one it captured
        del replay, out                                 # the graph goes only now, after its last replay has finished
    else:
        for i in range(steps):
            l = step()
            if i >= 1:
                losses.append(float(l.detach()))
        torch.cuda.synchronize()
    final = state.tolist()
    return losses, final, (step, net, flat, seed, x, state)


def test_captured_step_draws_a_new_mask_per_replay(dvt, device):
    eager, state_e, held_e = _training_run(dvt, device, 4, capture=False)
    graph, state_g, held_g = _training_run(dvt, device, 4, capture=True)
    print(f"[mae] three replayed losses {graph}; eager {eager}")
    assert len(set(graph)) > 1                          # the mask changes from replay to replay
    assert graph == eager
    b, n = 2, 16
    assert state_e == state_g == [77, 4 * ((b * n + 3) // 4)]
    torch.cuda.synchronize()
    del held_e, held_g
