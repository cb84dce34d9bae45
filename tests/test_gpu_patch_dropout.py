"""Patch dropout on the GPU (csrc/patch_dropout.hip, ops.keep_* / patchify_keep* / tokens_assemble_keep_*,
functional.patch_embed_keep / tokens_assemble_keep, ViViT(patch_dropout=) and ``keep=``) against the float64 CPU statement
tests/patchdrop_ref.py and the reference golden tests/golden/patch_dropout.npz.

Selection, drawing, gather and adjoint are integer work or permutations plus one rounding: exact.  Token assembly is one add
and one rounding per element: bit-equal to torch's; its backward on small-integer gradients: exact sums.  The model is held to
the project's per-operator bounds (tests/test_gpu_tubelet.py): rel-L2 <= 1e-4 in fp32 against the golden
of the imported reference, <= 1e-2 in bf16 / fp16 against ``patchdrop_ref.masked_step`` on the same dtype-rounded inputs.
No test here feeds an out-of-range index."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import patchdrop_ref as R
from tests import tubelet_ref as TR
from tests.util import fill_state_from_numpy, golden, rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
LP_TOL = 1e-2
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CANARY = 0x5A5A5A5A
FENCE = 64                                         # elements on either side of a raw output buffer


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


def _random_keys(R_, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (R_, n), generator=g, dtype=torch.int64).to(torch.int32)


# ---------------------------------------------------------------- selection
def _select_checked(dvt, device, keys, k, rows_per):
    """dvt_keep_select into fenced buffers, compared with the rank rule of the restatement."""
    R_, n = keys.shape
    kw, keep = _fenced(R_ * rows_per * k, torch.int32, -7, CANARY, device)
    sw, slot = _fenced(R_ * rows_per * n, torch.int32, -7, CANARY, device)
    kd = keys.to(device)
    lib = dvt._lib.load()
    dvt._lib.check(lib.dvt_keep_select(kd.data_ptr(), R_, n, k, rows_per, keep.data_ptr(), slot.data_ptr(), _stream()))
    torch.cuda.synchronize()
    ref_keep, ref_slot = R.keep_select(keys, k, rows_per)
    assert _fences_intact(kw, CANARY) and _fences_intact(sw, CANARY)
    assert torch.equal(keep.cpu().view(R_ * rows_per, k), ref_keep)
    assert torch.equal(slot.cpu().view(R_ * rows_per, n), ref_slot)
    # and through the wrapper
    k2, s2 = dvt.ops.keep_select(kd, k, rows_per)
    assert k2.dtype == s2.dtype == torch.int32 and torch.equal(k2.cpu(), ref_keep) and torch.equal(s2.cpu(), ref_slot)
    return ref_keep


def test_selection_ties_and_signed_order(dvt, device):
    keep = _select_checked(dvt, device, torch.zeros(3, 16, dtype=torch.int32), 5, 1)        # all-equal keys: 0 .. k-1
    assert torch.equal(keep, torch.arange(5, dtype=torch.int32).repeat(3, 1))
    keys = torch.tensor([[5, 1, 5, 1, 0, 7]], dtype=torch.int32)
    assert _select_checked(dvt, device, keys, 3, 2).tolist() == [[1, 3, 4]] * 2
    assert _select_checked(dvt, device, keys, 4, 2).tolist() == [[0, 1, 3, 4]] * 2          # the tie at 5: the lower position
    assert _select_checked(dvt, device, -keys, 1, 1).tolist() == [[5]]                      # signed order
    extremes = torch.tensor([[2 ** 31 - 1, -2 ** 31, 0, -1, 2 ** 31 - 1, -2 ** 31]], dtype=torch.int64).to(torch.int32)
    assert _select_checked(dvt, device, extremes, 3, 1).tolist() == [[1, 3, 5]]


SELECT_SHAPES = [(7, 196, 98), (3, 324, 81), (5, 16, 16), (5, 16, 1), (2, 1024, 512), (4, 100, 37)]


@pytest.mark.parametrize("rows_per", [1, 4])
@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_random_keys(dvt, device, shape, rows_per):
    R_, n, k = shape
    keep = _select_checked(dvt, device, _random_keys(R_, n, sum(shape)), k, rows_per)
    assert bool((keep[:, 1:] > keep[:, :-1]).all()) or k == 1


def test_slots_of_a_given_keep(dvt, device):
    keep, slot = R.keep_select(_random_keys(6, 100, 3), 37)
    assert torch.equal(dvt.ops.keep_slots(keep.to(device), 100).cpu(), slot)
    assert torch.equal(R.slots_of(keep, 100), slot)


# ---------------------------------------------------------------- drawing
def _state(device, seed=1130, base=0):
    return torch.tensor([seed, base], dtype=torch.int64, device=device)


@pytest.mark.parametrize("shape", [(64, 16, 8, 1), (3, 196, 98, 2), (2, 1024, 512, 1), (4, 100, 37, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_draw_is_the_selection_on_its_keys(dvt, device, shape):
    ops = dvt.ops
    R_, n, k, rows_per = shape
    st = _state(device)
    keys = ops.keep_keys(R_, n, st, 11)
    assert keys.shape == (R_, n) and keys.dtype == torch.int32
    keep, slot = ops.keep_draw(R_, n, k, st, 11, rows_per)
    rk, rs = R.keep_select(keys.cpu(), k, rows_per)
    assert torch.equal(keep.cpu(), rk) and torch.equal(slot.cpu(), rs)
    sk, ss = ops.keep_select(keys, k, rows_per)
    assert torch.equal(keep, sk) and torch.equal(slot, ss)
    again, _ = ops.keep_draw(R_, n, k, st, 11, rows_per)
    assert torch.equal(again, keep) and torch.equal(ops.keep_keys(R_, n, st, 11), keys)
    if k < n:
        other, _ = ops.keep_draw(R_, n, k, st, 12 + (R_ * n + 3) // 4, rows_per)
        assert not torch.equal(other, keep)
        ops.rng_advance_(st, 5 + (R_ * n + 3) // 4)
        advanced, _ = ops.keep_draw(R_, n, k, st, 11, rows_per)
        assert st.tolist() == [1130, 5 + (R_ * n + 3) // 4] and not torch.equal(advanced, keep)
        # the base and the call offset add up: the same counter, the same keys
        assert torch.equal(ops.keep_keys(R_, n, _state(device, base=7), 4), ops.keep_keys(R_, n, _state(device), 11))


def test_draw_uses_the_position(dvt, device):
    keep, slot = dvt.ops.keep_draw(64, 16, 8, _state(device), 0)
    keep = keep.cpu()
    assert keep.shape == (64, 8) and bool((keep[:, 1:] > keep[:, :-1]).all())
    assert int(keep.min()) >= 0 and int(keep.max()) < 16
    counts = torch.bincount(keep.reshape(-1).long(), minlength=16)
    print(f"[patch dropout] rows keeping each of 16 positions (of 64): {counts.tolist()}")
    assert int(counts.sum()) == 64 * 8
    # +- 5 sigma of Binomial(64, 1/2): sigma = 4; deterministic under the fixed seed
    assert int(counts.min()) >= 12 and int(counts.max()) <= 52
    assert len({tuple(r) for r in keep.tolist()}) > 32              # and the rows differ from one another


# ---------------------------------------------------------------- gather and adjoint
GATHER_SHAPES = [                                  # (b, t, C, H, W, P, pt, k)
    (2, 4, 3, 32, 32, 8, 2, 5),                    # vector form
    (2, 4, 3, 32, 32, 8, 1, 5),
    (1, 2, 3, 12, 12, 4, 1, 3),                    # scalar form
    (2, 8, 3, 64, 64, 16, 2, 7),                   # more than one wave per workgroup
    (2, 4, 3, 32, 32, 8, 2, 16),                   # k = n: the tubelet gather itself
    (1, 3, 3, 48, 16, 16, 1, 2),                   # P = 16: 6 kept patches of 2 per frame -- wave groups straddle frames, the last is partial
    (1, 3, 3, 48, 16, 16, 3, 2),                   # the same under pt = 3: the four vectors of a group at a 3 x 1536-byte stride
    (1, 4, 3, 64, 64, 16, 2, 16),                  # P = 16, k = n: the tubelet gather itself
]
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32")]


@functools.lru_cache(maxsize=None)
def _gather_case(shape):
    """(clip, keep, slot, gathered rows, a dout, its scatter, the kept-pixel mask), float64 small integers; never written."""
    b, t, C, H, W, P, pt, k = shape
    n = (H // P) * (W // P)
    x = TR.integer_clip((b, t, C, H, W), seed=sum(shape))
    keys = torch.from_numpy(np.random.default_rng(sum(shape) + 1).integers(0, 1000, (b * t // pt, n))).to(torch.int32)
    keep, slot = R.keep_select(keys, k)
    rows = R.gather_keep(x, P, pt, keep)
    y = TR.integer_clip(tuple(rows.shape), seed=sum(shape) + 2)
    back = R.scatter_keep(y, x.shape, P, pt, keep)
    mask = R.scatter_keep(torch.ones_like(rows), x.shape, P, pt, keep)
    return x, keep, slot, rows, y, back, mask


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kept_gather_and_adjoint_bit_exact(dvt, device, shape, pair):
    ops = dvt.ops
    b, t, C, H, W, P, pt, k = shape
    n = (H // P) * (W // P)
    src, dst = DT[pair[0]], DT[pair[1]]
    x, keep, slot, rows, y, back, mask = _gather_case(shape)
    xd, kd, sd = x.to(src).to(device), keep.to(device), slot.to(device)
    out = ops.patchify_keep(xd, P, pt, kd, dst)
    assert out.dtype == dst and out.shape == rows.shape
    assert torch.equal(out.cpu().double(), rows)
    if k == n:
        assert torch.equal(out, ops.tubelet_patchify(xd, P, pt, dst))
    lib = dvt._lib.load()
    # the same through the C entry into a fenced buffer: the kept rows and nothing around them
    fwhole, fout = _fenced(rows.numel(), dst, float("nan"), 77.0, device)
    dvt._lib.check(lib.dvt_patchify_keep(xd.data_ptr(), ops.dt(xd), fout.data_ptr(), ops.dt(fout), kd.data_ptr(), b * t, C, H, W,
                                         P, pt, k, _stream()))
    torch.cuda.synchronize()
    assert _fences_intact(fwhole, 77.0) and torch.equal(fout.view(out.shape), out)
    # the adjoint, straight through the C entry into a NaN-filled, fenced buffer: every pixel is written, nothing else
    whole, dx = _fenced(x.numel(), src, float("nan"), 77.0, device)
    yd = y.to(dst).to(device)
    dvt._lib.check(lib.dvt_patchify_keep_bwd(yd.data_ptr(), ops.dt(yd), dx.data_ptr(), ops.dt(dx), sd.data_ptr(), b * t, C, H, W,
                                             P, pt, k, _stream()))
    torch.cuda.synchronize()
    got = dx.cpu().double().view(x.shape)
    assert _fences_intact(whole, 77.0)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, back)
    assert bool((got[mask == 0] == 0).all()) and float(mask.mean()) == k / n
    via = ops.patchify_keep_bwd(yd, x.shape, P, pt, sd, src)
    assert via.dtype == src and torch.equal(via.cpu().double(), back)
    # <gather(x), y> == <x, adjoint(y)>, exactly on integer data
    assert float((out.cpu().double() * y).sum()) == float((x * got).sum())


def test_gather_ops_refuse_mismatched_tables(dvt, device):
    x = torch.zeros(2, 4, 3, 32, 32, device=device)
    keep = torch.zeros(3, 5, dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="shape"):
        dvt.ops.patchify_keep(x, 8, 2, keep, torch.float32)
    with pytest.raises(ValueError, match="tubelets"):
        dvt.ops.patchify_keep(x[:, :3], 8, 2, keep, torch.float32)
    with pytest.raises(ValueError, match="shape"):
        dvt.ops.patchify_keep_bwd(torch.zeros(20, 384, device=device), x.shape, 8, 2,
                                  torch.zeros(4, 15, dtype=torch.int32, device=device), torch.float32)


# ---------------------------------------------------------------- token assembly
ASSEMBLE_SHAPES = [(8, 4, 16, 5, 32, 2), (6, 3, 9, 9, 64, 0)]        # (S, T, n, k, d, positional rows above n + 1)


@functools.lru_cache(maxsize=None)
def _assemble_case(shape, tag):
    S, T, n, k, d, extra = shape
    g = torch.Generator().manual_seed(sum(shape))
    emb = torch.randn(S * k, d, generator=g).to(DT[tag])
    cls = torch.randn(d, generator=g)
    pos = torch.randn(T, n + 1 + extra, d, generator=g)
    keep, slot = R.keep_select(_random_keys(S, n, sum(shape) + 1), k)
    dout = torch.randint(-4, 5, (S, k + 1, d), generator=g).to(DT[tag])
    return emb, cls, pos, keep, slot, dout


def _assemble_ref(emb, cls, pos, keep, T):
    """float32 (or float64) adds, row by row, as the definition states them."""
    S, k = keep.shape
    rows = []
    for s in range(S):
        rows.append(cls + pos[s % T, 0])
        for i in range(k):
            rows.append(emb[s * k + i] + pos[s % T, 1 + int(keep[s, i])])
    return torch.stack(rows).reshape(S, k + 1, -1)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ASSEMBLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assembly_forward_bit_equal(dvt, device, shape, tag):
    S, T, n, k, d, extra = shape
    emb, cls, pos, keep, slot, _ = _assemble_case(shape, tag)
    out = dvt.ops.tokens_assemble_keep_fwd(emb.to(device), cls.to(device), pos.to(device), keep.to(device))
    assert out.shape == (S, k + 1, d) and out.dtype == DT[tag]
    assert torch.equal(out.cpu(), _assemble_ref(emb.float(), cls, pos, keep, T).to(DT[tag]))


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ASSEMBLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assembly_backward_exact_and_deterministic(dvt, device, shape, tag):
    ops = dvt.ops
    S, T, n, k, d, extra = shape
    emb, cls, pos, keep, slot, dout = _assemble_case(shape, tag)
    e64, c64, p64 = (v.double().requires_grad_() for v in (emb, cls, pos))
    _assemble_ref(e64, c64, p64, keep, T).backward(dout.double())
    dd, sd = dout.to(device), slot.to(device)
    demb, dcls, dpos = ops.tokens_assemble_keep_bwd(dd, T, n + 1 + extra, sd)
    assert demb.dtype == DT[tag] and dcls.dtype == dpos.dtype == torch.float32
    assert torch.equal(demb.cpu().double(), e64.grad) and torch.equal(dcls.cpu().double(), c64.grad)
    assert torch.equal(dpos.cpu().double(), p64.grad)
    # positions nobody kept (and the rows above n): exactly zero when overwriting ...
    kept = slot.reshape(S // T, T, n).ge(0).any(0)                                     # [T, n]
    idle = torch.ones(T, n + 1 + extra, dtype=torch.bool)
    idle[:, 0] = False
    idle[:, 1:n + 1] = ~kept
    assert bool(idle.any()) == (k < n or extra > 0)
    assert bool((dpos.cpu()[idle] == 0).all()) and not bool(torch.signbit(dpos.cpu()[idle]).any())
    # ... and exactly the pre-fill when accumulating
    acc_cls = torch.full((d,), 1.5, device=device)
    acc_pos = torch.full((T, n + 1 + extra, d), 3.25, device=device)
    acc_pos[0, -1, 0] = -0.0                                                            # an idle or kept element alike
    before = acc_pos.cpu().clone()
    demb2, c2, p2 = ops.tokens_assemble_keep_bwd(dd, T, n + 1 + extra, sd, dcls=acc_cls, dpos=acc_pos, accumulate=True)
    assert c2 is acc_cls and p2 is acc_pos and torch.equal(demb2, demb)
    assert torch.equal(acc_cls.cpu().double(), 1.5 + c64.grad)
    assert torch.equal(acc_pos.cpu().double(), before.double() + p64.grad)
    assert torch.equal(acc_pos.cpu()[idle].view(torch.int32), before[idle].view(torch.int32))
    # two runs are bitwise identical
    again = ops.tokens_assemble_keep_bwd(dd, T, n + 1 + extra, sd)
    assert all(torch.equal(a, b) for a, b in zip(again, (demb, dcls, dpos)))


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_functional_pair_against_float64_autograd(dvt, device, tag):
    """patch_embed_keep + tokens_assemble_keep with gradients to the clip, the weights, the CLS token and the table."""
    F = dvt.functional
    dtype = DT[tag]
    b, t, C, H, W, P, pt, k, d = 2, 4, 3, 32, 32, 8, 2, 5, 64
    n, S, T = 16, b * t // pt, t // pt
    K = pt * P * P * C
    g = torch.Generator().manual_seed(23)
    clip = torch.randn(b, t, C, H, W, generator=g).to(dtype).float()
    w = (torch.randn(d, K, generator=g) / K ** 0.5).to(dtype).float()
    bias = 0.1 * torch.randn(d, generator=g)
    cls, pos = 0.5 * torch.randn(1, 1, d, generator=g), 0.5 * torch.randn(1, T, n + 1, d, generator=g)
    keep, slot = R.keep_select(_random_keys(S, n, 29), k)
    dy = torch.randn(S, k + 1, d, generator=g).to(dtype)
    c64, w64, b64, cl64, p64 = (v.double().requires_grad_() for v in (clip, w, bias, cls, pos))
    e = R.gather_keep(c64, P, pt, keep) @ w64.t() + b64
    ref = _assemble_ref(e, cl64.reshape(-1), p64[0], keep, T)
    ref.backward(dy.double())
    cd, wd, bd, cld, pd_ = (v.to(device).requires_grad_() for v in (clip, w, bias, cls, pos))
    kd, sd = keep.to(device), slot.to(device)
    emb = F.patch_embed_keep(cd, wd, bd, P, dtype, pt, kd, sd)
    assert emb.shape == (S * k, d) and emb.dtype == dtype
    tok = F.tokens_assemble_keep(emb, cld, pd_, kd, sd, S, T)
    tok.backward(dy.to(device))
    errs = {"tok": rel_l2(tok, ref), "dclip": rel_l2(cd.grad, c64.grad), "dW": rel_l2(wd.grad, w64.grad),
            "db": rel_l2(bd.grad, b64.grad), "dcls": rel_l2(cld.grad, cl64.grad), "dpos": rel_l2(pd_.grad, p64.grad)}
    print(f"[patch dropout] patch_embed_keep + tokens_assemble_keep {tag}: {errs}")
    assert cd.grad.shape == clip.shape and pd_.grad.shape == pos.shape and cld.grad.shape == cls.shape
    assert all(v <= _tol(dtype) for v in errs.values()), errs


# ---------------------------------------------------------------- the model against the reference golden
@functools.lru_cache(maxsize=None)
def _golden():
    g = golden("patch_dropout.npz")
    cfg = {k[4:]: int(g[k]) for k in g.files if k.startswith("cfg_")}
    return g, cfg


def _golden_net(dtype, device, **kw):
    from dvt_amd.models.vit import ViViT
    g, cfg = _golden()
    net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"], compute_dtype=dtype, **kw)
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return net.to(device)


def _round_parameters_(net, dtype):
    """Weights a 16-bit kernel reads without a rounding of its own: the reference then sees the same values."""
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(dtype).float())


def _golden_inputs(device):
    g, cfg = _golden()
    clip, target, keep = (torch.from_numpy(g[k]) for k in ("clip", "target", "keep"))
    return clip, target, keep


def _check_step(tag, net, loss, logits, ref_logits, ref_loss, ref_grads, keep, tol, grad_scale=1.0):
    """``grad_scale``: the power of two backward was seeded with (an fp16 step is run under a loss scale, as the project
    trains in fp16: ``FlatParameters.enable_loss_scaling``); the fp32 master gradients are divided by it, exactly."""
    errs = {"logits": rel_l2(logits, ref_logits), "loss": abs(float(loss.detach()) - float(ref_loss)) / abs(float(ref_loss))}
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(ref_grads)
    for name, p in params.items():
        assert p.grad is not None and p.grad.shape == ref_grads[name].shape, name
        errs[name] = rel_l2(p.grad / grad_scale, ref_grads[name])
    worst = max(errs, key=errs.get)
    print(f"[patch dropout] model {tag}: loss {float(loss.detach()):.6f} / {float(ref_loss):.6f}; worst {worst} {errs[worst]:.2e}")
    # positional rows nobody kept: exactly zero
    S, k = keep.shape
    t = params["pos_embedding"].shape[1]
    n = params["pos_embedding"].shape[2] - 1
    kept = R.slots_of(keep, n).reshape(S // t, t, n).ge(0).any(0)
    gp = params["pos_embedding"].grad[0].cpu()
    assert not bool(kept.all()) and bool((gp[:, 1:][~kept] == 0).all()) and bool((gp[:, 1:][kept].abs().sum(-1) > 0).all())
    assert all(v <= tol for v in errs.values()), {k_: v for k_, v in errs.items() if v > tol}


def test_model_fp32_against_the_reference_golden(dvt, device):
    g, cfg = _golden()
    clip, target, keep = _golden_inputs(device)
    net = _golden_net(torch.float32, device).train()
    loss, logits = net.loss(clip.float().to(device), target.float().to(device), keep=keep.to(device))
    loss.backward()
    ref_grads = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("g:")}
    _check_step("fp32 / golden", net, loss, logits, torch.from_numpy(g["logits"]), float(g["loss"]), ref_grads, keep, F32_TOL)
    # eval with a caller's keep: the same logits (no dropout in this model), through forward()
    net.eval()
    with torch.no_grad():
        assert rel_l2(net(clip.float().to(device), keep=keep.to(device)), torch.from_numpy(g["logits"])) <= F32_TOL


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_model_16bit_against_the_restatement(dvt, device, tag):
    """fp16 runs under a loss scale of 1024 (a power of two: scaling and unscaling are exact).  Unscaled, the gradient that
    reaches the embedding is ~1e-5 per element here -- below fp16's smallest normal number, 6.1e-5, so it is stored with
    fewer than 11 bits -- and the patch weight's gradient measured 1.38e-2 where bf16, with a coarser mantissa but fp32's
    exponent range, measured 5.9e-3.  That is the format, and the reason the project trains fp16 under a loss scale."""
    g, cfg = _golden()
    dtype = DT[tag]
    clip, target, keep = _golden_inputs(device)
    clip = clip.to(dtype).double()
    net = _golden_net(dtype, device).train()
    _round_parameters_(net, dtype)
    P = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    ref_logits, ref_loss, ref_grads = R.masked_step(clip, target, P, keep, patch=cfg["patch"], depth=cfg["depth"],
                                                    heads=cfg["heads"])
    loss, logits = net.loss(clip.float().to(device), target.float().to(device), keep=keep.to(device))
    scale = 1024.0 if dtype == torch.float16 else 1.0
    loss.backward(torch.full((), scale, device=device))
    _check_step(tag + " / restatement", net, loss, logits, ref_logits, ref_loss, ref_grads, keep, LP_TOL, grad_scale=scale)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_tubelet_model_under_central_inflation(dvt, device, tag):
    from dvt_amd.models.vit import ViViT
    g, cfg = _golden()
    dtype = DT[tag]
    clip, target, keep = _golden_inputs(device)
    b = clip.shape[0]
    src = _golden_net(dtype, "cpu")
    tub = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"],
                dim_head=cfg["dim_head"], compute_dtype=dtype, tubelet_size=2)
    tub.load_frame_checkpoint(src.state_dict(), mode="central")
    tub = tub.to(device).train()
    if dtype != torch.float32:
        _round_parameters_(tub, dtype)
        clip = clip.to(dtype).double()
    keep2 = keep.reshape(b, cfg["frames"], -1)[:, 1::2].reshape(b * cfg["frames"] // 2, -1).contiguous()
    P = {k: v.detach().double().cpu() for k, v in tub.state_dict().items()}
    ref_logits, ref_loss, ref_grads = R.masked_step(clip, target, P, keep2, patch=cfg["patch"], depth=cfg["depth"],
                                                    heads=cfg["heads"], pt=2)
    loss, logits = tub.loss(clip.float().to(device), target.float().to(device), keep=keep2.to(device))
    loss.backward()
    _check_step(tag + " / pt = 2", tub, loss, logits, ref_logits, ref_loss, ref_grads, keep2, _tol(dtype))


# ---------------------------------------------------------------- identities
def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def test_keeping_every_position_is_the_plain_model(dvt, device):
    clip, target, _ = _golden_inputs(device)
    x, y = clip.float().to(device), target.float().to(device)
    net = _golden_net(torch.float32, device).train()
    n = net.num_patches
    every = torch.arange(n, dtype=torch.int32, device=device).repeat(x.shape[0] * net.num_frames, 1)
    loss_k, logits_k = net.loss(x, y, keep=every)
    loss_k.backward()
    gk = _grads(net)
    net.zero_grad(set_to_none=True)
    loss_p, logits_p = net.loss(x, y)
    loss_p.backward()
    assert torch.equal(logits_k, logits_p)
    errs = {k: rel_l2(gk[k], v) for k, v in _grads(net).items()}
    assert all(v <= F32_TOL for v in errs.values()), errs


def test_no_dropout_and_eval_are_the_default_model_bit_for_bit(dvt, device, monkeypatch):
    clip, target, _ = _golden_inputs(device)
    x, y = clip.float().to(device), target.float().to(device)
    default = _golden_net(torch.float32, device).train()
    zero = _golden_net(torch.float32, device, patch_dropout=0.0, patch_dropout_mode="frame").train()
    half = _golden_net(torch.float32, device, patch_dropout=0.5)
    drawn = []
    plain = dvt.ops.keep_draw
    monkeypatch.setattr(dvt.ops, "keep_draw", lambda *a, **k: drawn.append(1) or plain(*a, **k))
    la, za = default.loss(x, y)
    la.backward()
    lb, zb = zero.loss(x, y)
    lb.backward()
    assert torch.equal(za, zb) and torch.equal(la, lb)
    ga, gb = _grads(default), _grads(zero)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
    default.eval(), half.eval()
    with torch.no_grad():
        assert torch.equal(half(x), default(x))
    assert not drawn                                            # none of these drew a subset
    half.train()
    assert half.loss(x, y)[1].shape == za.shape and len(drawn) == 1
    dvt.functional.next_step()


@pytest.mark.parametrize("mode", ["tube", "frame"])
def test_tube_and_frame_modes(dvt, device, mode, monkeypatch):
    F = dvt.functional
    F.manual_seed(5)                                    # a fixed draw; no captured graph is alive here
    clip, target, _ = _golden_inputs(device)
    x, y = clip.float().to(device), target.float().to(device)
    net = _golden_net(torch.float32, device, patch_dropout=0.5, patch_dropout_mode=mode).train()
    seen = []
    plain = dvt.ops.keep_draw

    def tapped(*a, **k):
        r = plain(*a, **k)
        seen.append((a, r))
        return r

    monkeypatch.setattr(dvt.ops, "keep_draw", tapped)
    site = F._rng.site
    loss, logits = net.loss(x, y)
    loss.backward()
    (args, (keep, slot)), = seen
    b, t, n = x.shape[0], net.num_frames, net.num_patches
    assert keep.shape == (b * t, 8) and slot.shape == (b * t, n) and torch.equal(dvt.ops.keep_slots(keep, n), slot)
    rows = keep.cpu().view(b, t, 8)
    if mode == "tube":
        assert args[0] == b and bool((rows == rows[:, :1]).all()) and not torch.equal(rows[0, 0], rows[1, 0])
        assert F._rng.site - site == (b * n + 3) // 4
    else:
        assert args[0] == b * t and all(len({tuple(r) for r in clip_rows.tolist()}) > 1 for clip_rows in rows)
        assert F._rng.site - site == (b * t * n + 3) // 4
    # the step is the one a caller gets by passing the same keep
    g1 = _grads(net)
    net.zero_grad(set_to_none=True)
    loss2, logits2 = net.loss(x, y, keep=keep)
    loss2.backward()
    assert torch.equal(logits2, logits) and all(torch.equal(v, g1[k]) for k, v in _grads(net).items())
    F.next_step()


# ---------------------------------------------------------------- FlatParameters: sinks and no_sync
def test_flat_parameters_sinks_and_no_sync(dvt, device):
    from dvt_amd.dp import FlatParameters
    clip, target, keep1 = _golden_inputs(device)
    x, y = clip.float().to(device), target.float().to(device)
    n = 16
    keep2, _ = R.keep_select(_random_keys(keep1.shape[0], n, 41), 7)                   # another subset, another k
    k1, k2 = keep1.to(device), keep2.to(device)
    plain = _golden_net(torch.float32, device).train()
    separate = []
    for kp in (k1, k2):
        plain.zero_grad(set_to_none=True)
        plain.loss(x, y, keep=kp)[0].backward()
        separate.append(_grads(plain))
    net = _golden_net(torch.float32, device).train()
    flat = FlatParameters(net, compute_dtype=None)
    seed = torch.full((), flat.loss_scale, device=device)
    # one step with sinks
    flat.zero_grad()
    net.loss(x, y, keep=k1)[0].backward(seed)
    flat.finish_backward()
    errs = {k: rel_l2(p.grad, separate[0][k]) for k, p in net.named_parameters()}
    assert all(v <= F32_TOL for v in errs.values()), errs
    first_pos = net.pos_embedding.grad.clone()
    # a window of two micro-batches with different keeps: the sum of the two
    flat.zero_grad()
    with flat.no_sync():
        net.loss(x, y, keep=k1)[0].backward(seed)
        flat.finish_backward()
    assert torch.equal(net.pos_embedding.grad, first_pos)
    net.loss(x, y, keep=k2)[0].backward(seed)
    flat.finish_backward()
    errs = {k: rel_l2(p.grad, separate[0][k] + separate[1][k]) for k, p in net.named_parameters()}
    print(f"[patch dropout] no_sync window of two keeps: worst {max(errs.values()):.2e}")
    assert all(v <= F32_TOL for v in errs.values()), errs
    # positional rows the second micro-batch did not touch are the first one's, bit for bit
    S = keep2.shape[0]
    t = net.num_frames
    kept2 = R.slots_of(keep2, n).reshape(S // t, t, n).ge(0).any(0)
    kept1 = R.slots_of(keep1, n).reshape(S // t, t, n).ge(0).any(0)
    only_first = (kept1 & ~kept2)
    assert bool(only_first.any())
    now, then = net.pos_embedding.grad[0][:, 1:].cpu(), first_pos[0][:, 1:].cpu()
    assert torch.equal(now[~kept2], then[~kept2]) and bool((now[only_first].abs().sum(-1) > 0).all())
    assert bool((now[~kept1 & ~kept2] == 0).all())


# ---------------------------------------------------------------- a captured step draws a new subset on every replay
def _training_run(dvt, device, steps, capture):
    """Seed once, build, then ``steps`` steps of zero_grad; loss; backward; finish_backward; next_step -- eagerly, or one
    warm-up step and replays of the captured step.  Everything the captured graph addresses stays referenced from this frame
    until after the last replay and a synchronize."""
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    F = dvt.functional
    F.manual_seed(77)                                   # before anything is built; never between capture and replay
    clip, target, _ = _golden_inputs(device)
    x, y = clip.float().to(device), target.float().to(device)
    net = _golden_net(torch.float32, device, patch_dropout=0.5).train()
    flat = FlatParameters(net, compute_dtype=None)
    seed = torch.full((), flat.loss_scale, device=device)
    state = F._rng.tensor(x.device)

    def step(net=net, flat=flat, seed=seed, x=x, y=y):
        flat.zero_grad()
        loss, _ = net.loss(x, y)
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
    return losses, final, (step, net, flat, seed, x, y, state)


def test_captured_step_draws_a_new_subset_per_replay(dvt, device):
    eager, state_e, held_e = _training_run(dvt, device, 4, capture=False)
    graph, state_g, held_g = _training_run(dvt, device, 4, capture=True)
    print(f"[patch dropout] three replayed losses {graph}; eager {eager}")
    assert len(set(graph)) > 1                          # the subset changes from replay to replay
    assert graph == eager
    b, n = 2, 16
    assert state_e == state_g == [77, 4 * ((b * n + 3) // 4)]
    torch.cuda.synchronize()
    del held_e, held_g
