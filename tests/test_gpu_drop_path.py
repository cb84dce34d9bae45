"""Stochastic depth on the GPU (csrc/drop_path.hip, ops.seq_gather / seq_scatter_add / drop_path_draw,
functional.drop_path_block, ViViT(drop_path=, drop_path_mode=) and ``ViViT.drop_keep``) against the float64 CPU statement
tests/droppath_ref.py and the reference golden tests/golden/drop_path.npz.

The two streaming kernels are a row permutation, one multiply or fused multiply-add in fp32 and one rounding: bit-equal to the
reference on small integers with a power-of-two scale, within 1 ulp of the output type of the float64 result on general
values.  The model is held to the project's per-operator bounds (tests/test_gpu_patch_dropout.py):
rel-L2 <= 1e-4 in fp32 against the golden of the imported reference, <= 1e-2 in bf16 / fp16 against ``droppath_ref.step`` on
the same dtype-rounded inputs (fp16 under the loss scale the project trains fp16 with, as there).
No test here feeds an index outside [-1, bound)."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from tests import droppath_ref as R
from tests.util import fill_state_from_numpy, golden, rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
LP_TOL = 1e-2
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
MANT = {"f32": 23, "bf16": 7, "f16": 10}
EMIN = {"f32": -126, "bf16": -126, "f16": -14}
FENCE = 64                                         # elements on either side of a raw output buffer
FENCE_VALUE = 77.0
ALPHA = float(np.float32(12 / 11))                 # the scale as the kernel receives it (a C float)
# (S, k, L): the vector form; an odd length (scalar form); the identity; one kept row; a row longer than one workgroup pass
SHAPES = [(5, 3, 24), (5, 3, 35), (4, 4, 16), (6, 1, 8), (3, 2, 4104)]


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    assert (dvt_amd._lib.F32, dvt_amd._lib.BF16, dvt_amd._lib.F16) == (CODE["f32"], CODE["bf16"], CODE["f16"])
    return dvt_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fenced(numel, dtype, device):
    """A buffer of ``numel`` elements (NaN-filled) between two fences of FENCE elements -> (whole, the middle view)."""
    whole = torch.full((numel + 2 * FENCE,), FENCE_VALUE, dtype=dtype, device=device)
    mid = whole[FENCE:FENCE + numel]
    mid.fill_(float("nan"))
    return whole, mid


def _fences_intact(whole):
    return bool((whole[:FENCE] == FENCE_VALUE).all()) and bool((whole[-FENCE:] == FENCE_VALUE).all())


def _ulp(ref64: torch.Tensor, tag: str) -> torch.Tensor:
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** EMIN[tag]))).clamp_min(EMIN[tag])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[tag])


@functools.lru_cache(maxsize=None)
def _case(shape, integers):
    """(x [S, L], y [k, L], keep [k], slot [S], idx with one -1 where k > 1, its slot) in float64 -- made once per shape."""
    S, k, L = shape
    rng = np.random.default_rng(1000 * S + 10 * k + L + int(integers))
    if integers:
        x = torch.from_numpy(rng.integers(-8, 9, (S, L)).astype(np.float64))
        y = torch.from_numpy(rng.integers(-8, 9, (k, L)).astype(np.float64))
    else:
        x = torch.from_numpy(rng.standard_normal((S, L)))
        y = torch.from_numpy(rng.standard_normal((k, L)))
    keep = torch.from_numpy(np.sort(rng.permutation(S)[:k]).astype(np.int32))
    slot = R.slots_of(keep, S)
    idx, slot_d = keep.clone(), slot.clone()
    if k > 1:                                       # the documented "dropped" value in the middle of the list
        slot_d[int(idx[1])] = -1
        idx[1] = -1
    return x, y, keep, slot, idx, slot_d


def _gather_raw(dvt, x, idx, alpha, tag):
    S, L = x.shape
    k = idx.numel()
    whole, out = _fenced(k * L, x.dtype, x.device)
    lib = dvt._lib.load()
    dvt._lib.check(lib.dvt_seq_gather(x.data_ptr(), idx.data_ptr(), out.data_ptr(), S, k, L, alpha, CODE[tag], _stream()),
                   "dvt_seq_gather")
    torch.cuda.synchronize()
    assert _fences_intact(whole)
    return out.view(k, L).clone()


def _scatter_raw(dvt, res, y, slot, alpha, tag, in_place=False):
    S, L = res.shape
    k = y.shape[0]
    lib = dvt._lib.load()
    if in_place:
        whole, out = _fenced(S * L, res.dtype, res.device)
        out.copy_(res.reshape(-1))
        src = out
    else:
        whole, out = _fenced(S * L, res.dtype, res.device)
        src = res
    dvt._lib.check(lib.dvt_seq_scatter_add(src.data_ptr(), y.data_ptr(), slot.data_ptr(), out.data_ptr(), S, k, L, alpha,
                                           CODE[tag], _stream()), "dvt_seq_scatter_add")
    torch.cuda.synchronize()
    assert _fences_intact(whole)
    return out.view(S, L).clone()


# ---------------------------------------------------------------- the two kernels, through the C ABI
@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_bit_equal_on_integers_with_a_power_of_two_scale(dvt, device, shape, tag):
    x64, y64, keep, slot, idx, slot_d = _case(shape, True)
    dtype = DT[tag]
    x, y = x64.to(dtype).to(device), y64.to(dtype).to(device)
    for alpha in (1.0, 2.0, 0.5):
        for ix, sl in ((keep, slot), (idx, slot_d)):
            got = _gather_raw(dvt, x, ix.to(device), alpha, tag)
            want = R.gather(x64, ix, alpha).to(dtype)
            assert torch.equal(got.cpu(), want), ("gather", alpha)
            if ix is idx and shape[1] > 1:
                assert bool((got[1] == 0).all())                          # the dropped entry: a row of zeros
            want = R.scatter_add(x64, y64, sl, alpha).to(dtype)
            got = _scatter_raw(dvt, x, y, sl.to(device), alpha, tag)
            assert torch.equal(got.cpu(), want), ("scatter_add", alpha)
            again = _scatter_raw(dvt, x, y, sl.to(device), alpha, tag, in_place=True)
            assert torch.equal(again, got), ("in place", alpha)
    if shape[0] == shape[1]:                                              # the identity: keep names every row in order
        assert torch.equal(_gather_raw(dvt, x, keep.to(device), 1.0, tag), x)


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_within_one_ulp_on_general_values_and_repeatable(dvt, device, shape, tag):
    x64, y64, keep, slot, idx, slot_d = _case(shape, False)
    dtype = DT[tag]
    x, y = x64.to(dtype), y64.to(dtype)
    xd, yd = x.to(device), y.to(device)
    for ix, sl in ((keep, slot), (idx, slot_d)):
        got = _gather_raw(dvt, xd, ix.to(device), ALPHA, tag)
        ref = R.gather(x.double(), ix, ALPHA)
        err = ((got.cpu().double() - ref).abs() / _ulp(ref, tag)).max()
        print(f"[drop path] gather {shape} {tag}: {float(err):.3f} ulp")
        assert float(err) <= 1.0
        assert torch.equal(_gather_raw(dvt, xd, ix.to(device), ALPHA, tag), got)            # bitwise repeatable
        got = _scatter_raw(dvt, xd, yd, sl.to(device), ALPHA, tag)
        ref = R.scatter_add(x.double(), y.double(), sl, ALPHA)
        err = ((got.cpu().double() - ref).abs() / _ulp(ref, tag)).max()
        print(f"[drop path] scatter_add {shape} {tag}: {float(err):.3f} ulp")
        assert float(err) <= 1.0
        assert torch.equal(_scatter_raw(dvt, xd, yd, sl.to(device), ALPHA, tag), got)
        assert torch.equal(_scatter_raw(dvt, xd, yd, sl.to(device), ALPHA, tag, in_place=True), got)
        dropped = (sl < 0).nonzero().flatten()
        assert torch.equal(got.cpu()[dropped], x[dropped])                                   # a dropped row is res, bit for bit


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_ops_reach_the_vector_and_the_scalar_form(dvt, device, tag):
    """Through ops: an aligned row of 24 elements (16-byte accesses), the same data one element off a 16-byte line and a
    row of 35 (the scalar form) -- one result."""
    ops = dvt.ops
    x64, y64, keep, slot, _, _ = _case((5, 3, 24), True)
    dtype = DT[tag]
    kd, sd = keep.to(device), slot.to(device)
    x, y = x64.to(dtype).to(device), y64.to(dtype).to(device)
    want_g, want_s = R.gather(x64, keep, 2.0).to(dtype), R.scatter_add(x64, y64, slot, 2.0).to(dtype)
    assert torch.equal(ops.seq_gather(x.view(5, 3, 8), kd, 2.0).cpu().view(3, 24), want_g)
    assert torch.equal(ops.seq_scatter_add(x.view(5, 3, 8), y.view(3, 3, 8), sd, 2.0).cpu().view(5, 24), want_s)
    off_x = torch.zeros(5 * 24 + 8, dtype=dtype, device=device)[1:1 + 5 * 24].view(5, 24)
    off_y = torch.zeros(3 * 24 + 8, dtype=dtype, device=device)[1:1 + 3 * 24].view(3, 24)
    off_x.copy_(x), off_y.copy_(y)
    assert off_x.data_ptr() % 16 != 0 and off_x.is_contiguous()
    assert torch.equal(ops.seq_gather(off_x, kd, 2.0).cpu(), want_g)
    assert torch.equal(ops.seq_scatter_add(off_x, off_y, sd, 2.0).cpu(), want_s)
    out = ops.seq_scatter_add(off_x, off_y, sd, 2.0, out=off_x)                             # in place, through ops
    assert out is off_x and torch.equal(off_x.cpu(), want_s)
    x64, y64, keep, slot, _, _ = _case((5, 3, 35), True)
    got = ops.seq_gather(x64.to(dtype).to(device), keep.to(device), 0.5)
    assert torch.equal(got.cpu(), R.gather(x64, keep, 0.5).to(dtype))


def test_gather_and_scatter_add_are_adjoints_on_the_device(dvt, device):
    ops = dvt.ops
    for shape in SHAPES:
        x64, y64, keep, slot, idx, slot_d = _case(shape, True)
        x, y = x64.float().to(device), y64.float().to(device)
        for ix, sl in ((keep, slot), (idx, slot_d)):
            gx = ops.seq_gather(x, ix.to(device), 2.0)
            sy = ops.seq_scatter_add(torch.zeros_like(x), y, sl.to(device), 2.0)
            lhs = float((gx.cpu().double() * y64).sum())
            rhs = float((x64 * sy.cpu().double()).sum())
            assert lhs == rhs and lhs != 0.0, (shape, lhs, rhs)


# ---------------------------------------------------------------- draws
def _state(device, seed=1130, base=0):
    return torch.tensor([seed, base], dtype=torch.int64, device=device)


def test_bernoulli_draw(dvt, device):
    ops, F = dvt.ops, dvt.functional
    S = 1024
    st = _state(device, seed=9)
    m = ops.drop_path_draw(S, 0.25, st, 3)
    assert m.dtype == torch.int32 and m.shape == (S,)
    mc = m.cpu()
    pos = torch.arange(S, dtype=torch.int32)
    assert bool(((mc == pos) | (mc == -1)).all())                                   # s or -1 at position s
    assert torch.equal(ops.drop_path_draw(S, 0.25, st, 3), m)                       # a pure function of (state, offset)
    assert torch.equal(ops.drop_path_draw(S, 0.25, _state(device, seed=9), 3), m)
    assert not torch.equal(ops.drop_path_draw(S, 0.25, st, 3 + S // 4), m)          # another site
    assert not torch.equal(ops.drop_path_draw(S, 0.25, _state(device, seed=10), 3), m)
    kept = int((mc >= 0).sum())
    sd = math.sqrt(S * 0.25 * 0.75)
    print(f"[drop path] Bernoulli draw at S = 1024, p = 0.25: {kept} kept (768 +- {6 * sd:.0f})")
    assert abs(kept - 768) <= 6 * sd                                                # +- 83
    assert bool((ops.drop_path_draw(37, 0.0, st, 0).cpu() == torch.arange(37, dtype=torch.int32)).all())
    # through the generator: the same site reproduces, the next step differs
    F.manual_seed(21)
    state = F._rng.tensor(device)
    a = ops.drop_path_draw(S, 0.25, state, 0)
    assert torch.equal(ops.drop_path_draw(S, 0.25, state, 0), a)
    F._rng.take(S)
    F.next_step()
    b = ops.drop_path_draw(S, 0.25, state, 0)
    torch.cuda.synchronize()
    assert not torch.equal(a, b) and state.tolist() == [21, S // 4]
    F.manual_seed(1130)


@pytest.mark.parametrize("S,k", [(12, 7), (256, 231), (1024, 512), (3, 1), (8, 8)])
def test_subset_draw_is_ascending_unique_and_consistent(dvt, device, S, k):
    ops = dvt.ops
    st = _state(device, seed=5)
    keep, slot = ops.keep_draw(1, S, k, st, 0)
    assert keep.shape == (1, k) and slot.shape == (1, S) and keep.dtype == slot.dtype == torch.int32
    kc, sc = keep.cpu().view(k), slot.cpu().view(S)
    assert bool((kc[1:] > kc[:-1]).all()) and 0 <= int(kc[0]) and int(kc[-1]) < S
    assert torch.equal(sc, R.slots_of(kc, S))
    assert torch.equal(ops.keep_slots(keep, S), slot)
    if k < S:
        other, _ = ops.keep_draw(1, S, k, st, (S + 3) // 4)
        assert S < 8 or not torch.equal(other, keep)


# ---------------------------------------------------------------- the model against the reference golden
@functools.lru_cache(maxsize=None)
def _golden():
    g = golden("drop_path.npz")
    return (g,) + R.fixture(g)


def _net(dtype, device, **kw):
    from dvt_amd.models.vit import ViViT
    g, cfg = _golden()[:2]
    net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"], compute_dtype=dtype, **kw)
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return net.to(device)


def _grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def _on(device, keeps):
    return [None if e is None else e.to(device) for e in keeps]


@pytest.mark.parametrize("case", ["subset", "bernoulli"])
def test_model_fp32_against_the_reference_golden(dvt, device, case):
    g, cfg, clip, target, keeps, _ = _golden()
    net = _net(torch.float32, device, drop_path=float(g["drop_path"]), drop_path_mode=R.CASES[case][0]).train()
    net.drop_keep = _on(device, keeps)
    loss, logits = net.loss(clip.float().to(device), target.float().to(device))
    loss.backward()
    errs = R.digest_errors(g, case, logits, {k: p.grad for k, p in net.named_parameters()})
    errs["loss"] = abs(float(loss.detach()) - float(g[f"{case}:loss"])) / float(g[f"{case}:loss"])
    worst = max(errs, key=errs.get)
    print(f"[drop path] model fp32 / golden, {case}: loss {float(loss.detach()):.6f}; worst {worst} {errs[worst]:.2e}")
    assert len(errs) == len(list(net.parameters())) + 2
    assert all(v <= F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if v > F32_TOL}
    # what ran: per branch None or (keep, slot, alpha, gather) with the scale of the mode
    scales = R.alphas(keeps, 12, 3, cfg["depth"], float(g["drop_path"]), R.CASES[case][0])
    plan = net.last_drop_plan
    assert [None if e is None else e[2] for e in plan] == pytest.approx(scales)
    for e, kp in zip(plan, keeps):
        assert (e is None) == (kp is None)
        if e is not None:
            S = e[1].numel()
            assert torch.equal(e[0].cpu(), kp) and torch.equal(e[1].cpu(), R.slots_of(kp, S))


@pytest.mark.parametrize("case", ["subset", "bernoulli"])
@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_model_16bit_against_the_restatement(dvt, device, tag, case):
    """fp16 under a loss scale of 1024 (a power of two: exact), as tests/test_gpu_patch_dropout.py runs it and for its reason:
    unscaled, the gradient that reaches the embedding lies below fp16's smallest normal number."""
    g, cfg, clip, target, keeps, _ = _golden()
    dtype = DT[tag]
    mode = R.CASES[case][0]
    clip = clip.to(dtype).double()
    net = _net(dtype, device, drop_path=float(g["drop_path"]), drop_path_mode=mode).train()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(dtype).float())
    P = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    scales = R.alphas(keeps, 12, 3, cfg["depth"], float(g["drop_path"]), mode)
    ref_logits, ref_loss, ref_grads = R.step(clip, target, P, keeps, scales, patch=cfg["patch"], depth=cfg["depth"],
                                             heads=cfg["heads"])
    net.drop_keep = _on(device, keeps)
    loss, logits = net.loss(clip.float().to(device), target.float().to(device))
    scale = 1024.0 if dtype == torch.float16 else 1.0
    loss.backward(torch.full((), scale, device=device))
    errs = {"logits": rel_l2(logits, ref_logits), "loss": abs(float(loss.detach()) - float(ref_loss)) / float(ref_loss)}
    for name, p in net.named_parameters():
        errs[name] = rel_l2(p.grad / scale, ref_grads[name])
    worst = max(errs, key=errs.get)
    print(f"[drop path] model {tag} / restatement, {case}: worst {worst} {errs[worst]:.2e}")
    assert all(v <= LP_TOL for v in errs.values()), {k: v for k, v in errs.items() if v > LP_TOL}


def test_combined_with_patch_dropout_and_checkpointing(dvt, device):
    """Patch dropout through ``keep=``, dropout 0, every block checkpointed: within the bound of the golden, and the
    gradients of the un-checkpointed run bit for bit (the recomputation runs on the subsets the forward ran on)."""
    g, cfg, clip, target, keeps, patch_keep = _golden()
    x, y = clip.float().to(device), target.float().to(device)
    runs = {}
    for ckpt in (False, True):
        net = _net(torch.float32, device, drop_path=float(g["drop_path"]), activation_checkpointing=ckpt).train()
        net.drop_keep = _on(device, keeps)
        loss, logits = net.loss(x, y, keep=patch_keep.to(device))
        loss.backward()
        runs[ckpt] = (logits, _grads(net))
    errs = R.digest_errors(g, "combined", runs[True][0], runs[True][1])
    worst = max(errs, key=errs.get)
    print(f"[drop path] combined with patch dropout, checkpointed: worst {worst} {errs[worst]:.2e}")
    assert all(v <= F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if v > F32_TOL}
    assert torch.equal(runs[True][0], runs[False][0])
    assert all(torch.equal(v, runs[False][1][k]) for k, v in runs[True][1].items())


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_inactive_cases_are_the_plain_model_bit_for_bit(dvt, device, tag, monkeypatch):
    g, cfg, clip, target, keeps, _ = _golden()
    dtype = DT[tag]
    x, y = clip.float().to(device), target.float().to(device)
    plain = _net(dtype, device).train()
    dp = _net(dtype, device, drop_path=0.3)
    dp.load_state_dict(plain.state_dict())
    calls = []
    for name in ("seq_gather", "seq_scatter_add", "drop_path_draw", "keep_draw"):
        fn = getattr(dvt.ops, name)
        monkeypatch.setattr(dvt.ops, name, lambda *a, _f=fn, _n=name, **k: calls.append(_n) or _f(*a, **k))
    lp, zp = plain.loss(x, y)
    lp.backward()
    gp = _grads(plain)
    dp.train()
    dp.drop_keep = [None] * 8                                   # training, every branch on all sequences
    ld, zd = dp.loss(x, y)
    ld.backward()
    assert torch.equal(zd, zp) and torch.equal(ld, lp)
    assert all(torch.equal(v, gp[k]) for k, v in _grads(dp).items())
    assert dp.last_drop_plan == [None] * 8
    dp.drop_keep = None
    dp.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(dp(x), plain(x))
    assert dp.last_drop_plan is None and not calls              # the new code was not reached
    dp.train()
    assert dp.loss(x, y)[1].shape == zp.shape and "seq_scatter_add" in calls
    dvt.functional.next_step()


@pytest.mark.parametrize("mode", ["subset", "bernoulli"])
def test_drawn_on_the_device(dvt, device, mode):
    """A step with the subsets drawn on the device, read back from ``last_drop_plan``: ``subset`` -- k = S - floor(p S) rows,
    the step a caller gets by passing the same subsets, bit for bit; ``bernoulli`` -- the restatement with the drawn masks."""
    F = dvt.functional
    F.manual_seed(6)                                            # a fixed draw; no captured graph is alive here
    g, cfg, clip, target, _, _ = _golden()
    x, y = clip.float().to(device), target.float().to(device)
    net = _net(torch.float32, device, drop_path=0.5, drop_path_mode=mode).train()
    rates = net.space_transformer.drop_path_rates + net.temporal_transformer.drop_path_rates
    site = F._rng.site
    loss, logits = net.loss(x, y)
    loss.backward()
    plan = net.last_drop_plan
    assert len(plan) == 8 and math.isfinite(float(loss.detach()))
    S_of = [12] * 4 + [3] * 4
    drawn = 0
    keeps = []
    for j, (e, S) in enumerate(zip(plan, S_of)):
        p = rates[j // 2 if j < 4 else 2 + (j - 4) // 2]
        if mode == "subset":
            k = S - math.floor(p * S)
            assert (e is None) == (k == S), j
            if e is not None:
                kp = e[0].cpu()
                assert kp.numel() == k and bool((kp[1:] > kp[:-1]).all()) and e[2] == S / k and e[3]
                assert torch.equal(e[1].cpu(), R.slots_of(kp, S))
                drawn += 1
            keeps.append(None if e is None else e[0])
        else:
            assert (e is None) == (p == 0.0), j
            if e is not None:
                m = e[0].cpu()
                assert e[0] is e[1] and not e[3] and e[2] == pytest.approx(1 / (1 - p))
                assert bool(((m == torch.arange(S, dtype=torch.int32)) | (m == -1)).all())
                drawn += 1
            keeps.append(None if e is None else e[0].cpu()[e[0].cpu() >= 0])
    assert drawn >= 4 and F._rng.site - site == sum((S + 3) // 4 for e, S in zip(plan, S_of) if e is not None)
    if mode == "subset":
        g1 = _grads(net)
        net.zero_grad(set_to_none=True)
        net.drop_keep = keeps
        loss2, logits2 = net.loss(x, y)
        loss2.backward()
        assert torch.equal(logits2, logits) and all(torch.equal(v, g1[k]) for k, v in _grads(net).items())
    else:
        P = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
        scales = [None if e is None else e[2] for e in plan]
        ref_logits, ref_loss, ref_grads = R.step(clip, target, P, keeps, scales, patch=cfg["patch"], depth=cfg["depth"],
                                                 heads=cfg["heads"])
        errs = {"logits": rel_l2(logits, ref_logits)}
        for name, p in net.named_parameters():
            errs[name] = rel_l2(p.grad, ref_grads[name])
        worst = max(errs, key=errs.get)
        print(f"[drop path] drawn Bernoulli masks against the restatement: worst {worst} {errs[worst]:.2e}")
        assert all(v <= F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if v > F32_TOL}
    F.next_step()


@pytest.mark.parametrize("mode", ["subset", "bernoulli"])
def test_composes_with_dropout_tubelets_and_checkpointing(dvt, device, mode):
    """dropout 0.1 (the blocks' unfused route inside the branch), tubelet_size 2 (S = 6 in the space stack), drawn subsets:
    the checkpointed step repeats the un-checkpointed one bit for bit -- the recomputation draws no site again, neither a
    subset's nor a dropout mask's -- and another seed gives another step."""
    from dvt_amd.models.vit import ViViT
    F = dvt.functional
    g, cfg, clip, target, _, _ = _golden()
    x, y = clip.float().to(device), target.float().to(device)
    runs = []
    for seed, ckpt in ((31, False), (31, True), (32, False)):
        F.manual_seed(seed)                                     # no captured graph is alive here
        torch.manual_seed(3)
        net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                    heads=cfg["heads"], dim_head=cfg["dim_head"], compute_dtype=torch.float32, dropout=0.1, drop_path=0.5,
                    drop_path_mode=mode, tubelet_size=2, activation_checkpointing=ckpt).to(device).train()
        loss, logits = net.loss(x, y)
        loss.backward()
        plan = net.last_drop_plan
        assert sum(e is not None for e in plan) >= 4 and all(e is None or e[1].numel() in (6, 3) for e in plan)
        assert math.isfinite(float(loss.detach())) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        runs.append((logits, _grads(net)))
        F.next_step()
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(v, runs[1][1][k]) for k, v in runs[0][1].items())
    assert not torch.equal(runs[0][0], runs[2][0])
    F.manual_seed(1130)


# ---------------------------------------------------------------- a captured step draws new subsets on every replay
def _training_run(dvt, device, steps, capture):
    """Seed once, build, then ``steps`` steps of zero_grad; loss; backward; finish_backward; next_step -- eagerly, or one
    warm-up step and replays of the captured step.  Everything the captured graph addresses stays referenced from this frame
    until after the last replay and a synchronize."""
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    F = dvt.functional
    F.manual_seed(78)                                   # before anything is built; never between capture and replay
    g, cfg, clip, target, _, _ = _golden()
    x, y = clip.float().to(device), target.float().to(device)
    net = _net(torch.float32, device, drop_path=0.5).train()
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

    def subsets():
        return [None if e is None else e[0].cpu().tolist() for e in net.last_drop_plan]

    losses, seen = [], []
    if capture:
        replay, out = capture_step(step, warmup=1)
        for _ in range(steps - 1):
            replay()
            losses.append(float(out.detach()))
            seen.append(subsets())
        torch.cuda.synchronize()
        assert F._rng.state is state                    # the generator state the graph addresses is still the one it captured
        del replay, out                                 # the graph goes only now, after its last replay has finished
    else:
        for i in range(steps):
            l = step()
            if i >= 1:
                losses.append(float(l.detach()))
                seen.append(subsets())
        torch.cuda.synchronize()
    return losses, seen, state.tolist(), (step, net, flat, seed, x, y, state)


def test_captured_step_draws_new_subsets_per_replay(dvt, device):
    eager, seen_e, state_e, held_e = _training_run(dvt, device, 4, capture=False)
    graph, seen_g, state_g, held_g = _training_run(dvt, device, 4, capture=True)
    print(f"[drop path] three replayed losses {graph}; eager {eager}")
    assert len(graph) == 3 and all(math.isfinite(v) for v in graph)
    live = [j for j, e in enumerate(seen_g[0]) if e is not None]
    assert live and any(len({tuple(s[j]) for s in seen_g}) > 1 for j in live)       # a branch's subset changes per replay
    assert seen_g == seen_e and graph == eager                  # the same seed and step: the same subsets, the same loss bits
    again, seen_a, state_a, held_a = _training_run(dvt, device, 2, capture=True)
    assert again[0] == graph[0] and seen_a[0] == seen_g[0]      # replaying from the same seed and step reproduces the first
    sites = sum((S + 3) // 4 for e, S in zip(seen_g[0], [12] * 4 + [3] * 4) if e is not None)
    assert state_e == state_g == [78, 4 * sites]
    torch.cuda.synchronize()
    del held_e, held_g, held_a
