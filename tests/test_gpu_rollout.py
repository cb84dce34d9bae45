"""Attention rollout on the GPU (csrc/attn_rollout.hip, dvt_amd/rollout.py, functional.attention_tap) against the float64
restatement tests/rollout_ref.py, which multiplies full matrices -- not the vector recurrence the kernels use.

The kernel bound.  Both sides get the same 16-bit (or fp32) Q and K; the lse is the restatement's float64 one rounded to
fp32.  With |scale q.k| <= 20 the fp32 dot product of dh <= 448 terms and the fp32 lse put at most about
dh 2^-24 20 <= 5e-4 (typically 1e-5) of absolute error into the exponent; the exponential turns that into a relative error
of each probability, and the sums have non-negative weights: |out - ref| <= 2e-4 max(ref) per sequence."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import rollout_ref as R
from tests.util import fill_state_from_numpy, golden

rel_l2 = R.rel_l2                                     # tensors or arrays, any device

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
STEP_BOUND = 2e-4
RHO = 0.5


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


# ---------------------------------------------------------------- inputs
def _qk(S, H, N, dh, dtype, seed, smax=15.0):
    """Packed qkv [S, N, 3, H, dh] of `dtype` (CPU) with max |scale q.k| = smax before rounding -> (qkv, q view, k view)."""
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.standard_normal((S, N, 3, H, dh)))
    scale = dh ** -0.5
    s = torch.einsum("sihd,sjhd->shij", a[:, :, 0], a[:, :, 1]) * scale
    a[:, :, 0] *= smax / float(s.abs().max())
    qkv = a.to(dtype)
    q, k = qkv[:, :, 0].permute(0, 2, 1, 3), qkv[:, :, 1].permute(0, 2, 1, 3)
    assert float((torch.einsum("shid,shjd->shij", q.double(), k.double()) * scale).abs().max()) <= 20.0
    return qkv, q, k


def _dev_views(qkv, device):
    d = qkv.to(device)
    return d, d[:, :, 0].permute(0, 2, 1, 3), d[:, :, 1].permute(0, 2, 1, 3)


def _start(S, N, seed):
    r = torch.from_numpy(np.random.default_rng(seed).random((S, N)) + 0.05)
    return (r / r.sum(1, keepdim=True)).float()


def _check(out, ref, what):
    out = out.double().cpu()
    err = (out - ref).abs().amax(1) / ref.amax(1)
    print(f"[rollout] {what}: worst |out - ref| / max(ref) = {float(err.max()):.2e}, row sums off by "
          f"{float((out.sum(1) - 1).abs().max()):.2e}")
    assert torch.isfinite(out).all()
    assert float(err.max()) <= STEP_BOUND, what
    assert float((out.sum(1) - 1.0).abs().max()) <= 1e-5, what


STEP_CASES = [(1, 1, 16, 64), (3, 2, 17, 64), (2, 3, 33, 64), (2, 8, 197, 64), (1, 2, 325, 64), (1, 1, 352, 64), (1, 1, 353, 64)]
STEP_IDS = [f"{s}x{h}x{n}" for s, h, n, _ in STEP_CASES]
GENERIC_CASES = [(2, 2, 14, 448, "f32"), (2, 2, 14, 448, "bf16"), (3, 4, 5, 32, "f32"), (2, 2, 17, 64, "f32")]


def _run_step_case(dvt, device, S, H, N, dh, tag, form):
    ops = dvt.ops
    qkv, q, k = _qk(S, H, N, dh, DT[tag], seed=1000 + N + dh)
    scale = dh ** -0.5
    lse = R.lse(q, k, scale).float().contiguous()
    r_in = _start(S, N, seed=7 + N)
    _, qd, kd = _dev_views(qkv, device)
    lse_d, r_d = lse.to(device), r_in.to(device)
    plan = ops.rollout_plan(qd, kd, r_d)
    assert plan.form in ("mfma", "generic") and (form is None or plan.form == form), plan
    out = ops.rollout_step(qd, kd, lse_d, r_d, residual=RHO)
    assert out.shape == (S, N) and out.dtype == torch.float32
    _check(out, R.step(q, k, scale, r_in, RHO), f"{tag} {S}x{H}x{N}x{dh} random start ({plan.form}, {plan.waves} waves)")
    # one-hot start without a stored vector, and the same layer run for that query alone (Lq == 1)
    one = ops.rollout_step(qd, kd, lse_d, None, query=0, residual=RHO)
    _check(one, R.rollout([(q, k, scale)], RHO, query=0), f"{tag} {S}x{H}x{N}x{dh} query=0")
    q1 = ops.rollout_step(qd[:, :, :1], kd, lse_d[:, :, :1].contiguous(), None, query=0, residual=RHO)
    assert torch.equal(q1, one)
    return qd, kd, lse_d, r_d


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_step_mfma_form(dvt, device, case, tag):
    S, H, N, dh = case
    # 353 keys: one past the forward kernel's register-tile limit; it takes whatever form the plan names (both are held
    # to the same bound), every shorter one the MFMA form
    _run_step_case(dvt, device, S, H, N, dh, tag, None if N > 352 else "mfma")


@pytest.mark.parametrize("case", GENERIC_CASES, ids=[f"{s}x{h}x{n}x{d}-{t}" for s, h, n, d, t in GENERIC_CASES])
def test_step_generic_form(dvt, device, case):
    S, H, N, dh, tag = case
    _run_step_case(dvt, device, S, H, N, dh, tag, "generic")


def test_step_uniform_start_and_other_residuals(dvt, device):
    ops = dvt.ops
    for (S, H, N, dh, tag) in ((2, 2, 33, 64, "bf16"), (2, 2, 14, 448, "f32")):
        qkv, q, k = _qk(S, H, N, dh, DT[tag], seed=55 + N)
        scale = dh ** -0.5
        _, qd, kd = _dev_views(qkv, device)
        lse_d = R.lse(q, k, scale).float().contiguous().to(device)
        for rho in (0.0, 0.25, 1.0):
            out = ops.rollout_step(qd, kd, lse_d, None, query=ops.ROLLOUT_UNIFORM, residual=rho)
            _check(out, R.rollout([(q, k, scale)], rho, query=None), f"{tag} uniform start, residual {rho}")
        # a scale other than dh^-1/2 is passed on
        out = ops.rollout_step(qd, kd, R.lse(q, k, 0.5 * scale).float().contiguous().to(device), _start(S, N, 3).to(device),
                               residual=RHO, scale=0.5 * scale)
        _check(out, R.step(q, k, 0.5 * scale, _start(S, N, 3), RHO), f"{tag} half scale")


# ---------------------------------------------------------------- orientation
@pytest.mark.parametrize("tag", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", [1, 2])
def test_orientation_with_permutation_matrices(dvt, device, H, tag):
    """Every P is a permutation matrix (score 0 on the chosen key, -200 elsewhere: the exponential is exactly 0 in fp32), a
    5-cycle, which is not its own inverse: r P and P r differ in every entry.  Catches a transposed reduction."""
    ops = dvt.ops
    N, dh = 5, 64
    perms = [torch.tensor([1, 2, 3, 4, 0]), torch.tensor([2, 3, 4, 0, 1])][:H]
    qkv = torch.zeros(1, N, 3, H, dh, dtype=torch.float64)
    for h, perm in enumerate(perms):
        for i in range(N):
            qkv[0, i, 0, h, i] = 1.0                  # q_i = e_i
            qkv[0, :, 1, h, i] = -200.0               # k_j[i] = -200 ...
            qkv[0, perm[i], 1, h, i] = 0.0            # ... but 0 on the key query i attends to
    qkv = qkv.to(DT[tag])
    q, k = qkv[:, :, 0].permute(0, 2, 1, 3), qkv[:, :, 1].permute(0, 2, 1, 3)
    r_in = (torch.tensor([[16.0, 8.0, 4.0, 2.0, 1.0]]) / 31.0).float()
    ref = R.step(q, k, 1.0, r_in, 0.25)
    want = 0.25 * r_in.double()
    for perm in perms:
        for i in range(N):
            want[0, perm[i]] += 0.75 / H * r_in.double()[0, i]
    assert float((ref - want).abs().max()) <= 1e-15
    transposed = 0.25 * r_in.double() + 0.75 * torch.einsum("shij,sj->si", R.probs(q, k, 1.0).mean(1, keepdim=True), r_in.double())
    assert float((ref - transposed).abs().min()) > 1e-3
    _, qd, kd = _dev_views(qkv, device)
    lse = torch.zeros(1, H, N, dtype=torch.float32, device=device)         # log(1 + 4 e^-200) == 0 in fp32
    assert ops.rollout_plan(qd, kd, r_in.to(device), scale=1.0).form == ("generic" if tag == "f32" else "mfma")
    out = ops.rollout_step(qd, kd, lse, r_in.to(device), residual=0.25, scale=1.0)
    assert float((out.double().cpu() - ref).abs().max()) <= 1e-6


# ---------------------------------------------------------------- the start from the folded layer's probabilities
def test_from_probs_after_the_real_folded_forward(dvt, device):
    ops = dvt.ops
    S, N, d, H, dh, eps = 3, 17, 128, 2, 64, 1e-5
    rng = np.random.default_rng(17)
    x = torch.from_numpy(rng.standard_normal((S, N, d))).to(torch.bfloat16)
    gamma = torch.from_numpy(1 + 0.1 * rng.standard_normal(d)).float()
    beta = torch.from_numpy(0.1 * rng.standard_normal(d)).float()
    wk = torch.from_numpy(rng.standard_normal((H, dh, d)) / np.sqrt(d))
    qv = torch.from_numpy(rng.standard_normal((S, H, dh)))
    scale = dh ** -0.5
    xd = x.double()
    ln = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()
    kmat = torch.einsum("hed,sjd->shje", wk, ln)                                   # K = Wk LN(x) [S, H, N, dh]
    smax = float((torch.einsum("she,shje->shj", qv, kmat) * scale).abs().max())
    qv *= 12.0 / smax                                                              # max |s| = 12 <= 20
    Rm = (scale * torch.einsum("she,hed->shd", qv, wk)).float().contiguous()       # r_h = scale Wk_h^T q_h
    xdev = x.to(device)
    assert ops.attn_cls_supported(xdev, H, dh)
    _, lse, P, _, _ = ops.attn_cls_fwd(xdev, gamma.to(device), beta.to(device), eps, Rm.to(device))
    assert P.shape == (S, N, 8)
    out = ops.rollout_from_probs(P, H, query=0, residual=RHO)
    qfull = torch.zeros(S, H, N, dh, dtype=torch.float64)
    qfull[:, :, 0] = qv                                                            # only the CLS query is ever read
    ref = R.rollout([(qfull, kmat, scale)], RHO, query=0)
    _check(out, ref, "from_probs after attn_cls_fwd")
    # the same start from q, K and lse of that layer (the unfolded single-query form): one query row
    k16 = kmat.to(torch.bfloat16)
    q16 = qv.to(torch.bfloat16).view(S, H, 1, dh)
    lse1 = torch.logsumexp(torch.einsum("shie,shje->shij", q16.double(), k16.double()) * scale, -1).float()
    one = ops.rollout_step(q16.to(device), k16.to(device).contiguous(), lse1.contiguous().to(device), None, query=0, residual=RHO)
    qfull[:, :, 0] = q16.double().view(S, H, dh)
    _check(one, R.rollout([(qfull, k16, scale)], RHO, query=0), "Lq == 1 step")


# ---------------------------------------------------------------- the video launch
@pytest.mark.parametrize("B,T,n", [(3, 3, 16), (2, 5, 100)])
def test_video_launch_is_exact(dvt, device, B, T, n):
    """Products m / c x c with c in {0.5, 1, 2} and m a multiple of 1/4 in [3, 11] are exact; every clip holds a 3 and an 11,
    so max - min = 8 swallows the 1e-7 of the denominator in fp32 and the quotients are dyadic: bitwise comparison with the
    float64 restatement rounded once."""
    rng = np.random.default_rng(B * 100 + n)
    m = rng.integers(12, 45, (B, T, n)) / 4.0
    m[:, 0, 1], m[:, T - 1, n - 2] = 3.0, 11.0
    c = rng.choice([0.5, 1.0, 2.0], (B, T))
    r_time = np.concatenate([np.full((B, 1), 100.0), c], 1)
    r_space = np.concatenate([np.full((B, T, 1), -7.0), m / c[:, :, None]], 2).reshape(B * T, n + 1)
    rs, rt = torch.from_numpy(r_space).float(), torch.from_numpy(r_time).float()
    assert torch.equal(rs.double(), torch.from_numpy(r_space)) and torch.equal(rt.double(), torch.from_numpy(r_time))
    raw, scaled = dvt.ops.rollout_video(rs.to(device), rt.to(device))
    _, _, vid, sc = R.video(rs, rt)
    assert torch.equal(raw.cpu(), vid.float()) and torch.equal(vid.float().double(), vid)
    assert torch.equal(scaled.cpu(), sc.float())
    assert float(scaled.min()) == 0.0 and float(scaled.max()) == 1.0
    assert dvt.ops.rollout_video(rs.to(device), rt.to(device), want_raw=False)[0] is None


# ---------------------------------------------------------------- repeatability
def test_every_launch_is_repeatable(dvt, device):
    ops = dvt.ops
    S, H, N, dh = 2, 8, 197, 64
    for tag in ("bf16", "f32"):
        qkv, q, k = _qk(S, H, N, dh, DT[tag], seed=99)
        _, qd, kd = _dev_views(qkv, device)
        lse = R.lse(q, k, dh ** -0.5).float().contiguous().to(device)
        r = _start(S, N, 5).to(device)
        for kw in (dict(r_in=r), dict(r_in=None, query=0), dict(r_in=None, query=ops.ROLLOUT_UNIFORM)):
            a, b = ops.rollout_step(qd, kd, lse, **kw), ops.rollout_step(qd, kd, lse, **kw)
            assert torch.equal(a, b), (tag, kw.keys())
    P = torch.from_numpy(np.random.default_rng(3).random((S, N, 8))).float().to(device)
    assert torch.equal(ops.rollout_from_probs(P, H), ops.rollout_from_probs(P, H))
    rs, rt = _start(S * 8, N, 11).to(device), _start(S, 9, 12).to(device)
    a, b = ops.rollout_video(rs, rt), ops.rollout_video(rs, rt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- end to end: ViViT against the reference fixture
def _fixture_model(dvt, fx, dtype, **over):
    from dvt_amd.models.vit import ViViT
    cfg = {k[4:]: int(fx[k]) for k in fx.files if k.startswith("cfg_")}
    cfg.update(over)
    net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"], pool=cfg.get("pool", "cls"), compute_dtype=dtype)
    fill_state_from_numpy(net.named_parameters(), int(fx["fill_seed"]))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("to_qkv.weight"):
                p.mul_(float(fx["qkv_gain"]))
    return net


@pytest.fixture(scope="module")
def fx():
    return golden("attention_rollout.npz")


def _e2e(dvt, device, fx, dtype):
    from dvt_amd.rollout import AttentionRollout
    net = _fixture_model(dvt, fx, dtype).to(device)
    clip = torch.from_numpy(fx["clip"]).to(device)
    ro = AttentionRollout(net, residual=float(fx["rho"]))
    r_space, r_time = ro.rows(clip)
    space, time, video = ro.maps(clip)
    b, t = clip.shape[0], clip.shape[1]
    assert ro.outputs.shape == (b, int(fx["cfg_classes"])) and space.shape == video.shape == (b, t, 4, 4) and time.shape == (b, t)
    assert torch.equal(space.reshape(b * t, -1), r_space[:, 1:]) and torch.equal(time, r_time[:, 1:])
    return {"r_space": rel_l2(r_space, fx["r_space"]), "r_time": rel_l2(r_time, fx["r_time"]),
            "video": rel_l2(video.reshape(b, t, -1), fx["video"])}


def test_vivit_fp32_against_the_reference_fixture(dvt, device, fx):
    errs = _e2e(dvt, device, fx, torch.float32)
    print(f"[rollout] ViViT fp32 against the reference's float64 rollout: {errs}")
    assert all(v <= 1e-3 for v in errs.values()), errs              # the fp32 protocol bound


@pytest.mark.parametrize("tag", ["bf16", "fp16"])
def test_vivit_16bit_within_twice_the_references_own_deviation(dvt, device, fx, tag):
    errs = _e2e(dvt, device, fx, torch.bfloat16 if tag == "bf16" else torch.float16)
    own = {k: float(fx[f"{tag}:{k}_err"]) for k in errs}
    print(f"[rollout] ViViT {tag}: {errs}; the reference's own {tag}: {own}")
    assert all(errs[k] <= 2 * own[k] for k in errs), (errs, own)


def test_vivit_folded_last_layer_starts_from_probs(dvt, device, fx, monkeypatch):
    """The space stack's last layer on the folded single-query path (forced at this small shape): the start of the recurrence
    is rollout_from_probs; same bound as the unfolded bf16 run."""
    from dvt_amd import functional as F
    monkeypatch.setattr(F, "CLS_FOLD_MIN_ROWS", 1)
    net = _fixture_model(dvt, fx, torch.bfloat16).to(device).eval()
    clip = torch.from_numpy(fx["clip"]).to(device)
    with torch.no_grad(), F.attention_tap() as layers:
        net(clip)
    assert [t.kind for t in layers] == ["dense", "dense", "folded", "dense", "dense", "cls"]
    errs = _e2e(dvt, device, fx, torch.bfloat16)
    own = {k: float(fx[f"bf16:{k}_err"]) for k in errs}
    print(f"[rollout] ViViT bf16, folded last space layer: {errs}; the reference's own bf16: {own}")
    assert all(errs[k] <= 2 * own[k] for k in errs), (errs, own)


def _layers_of(taps):
    """Taps -> [(q, k, scale)] on the CPU in float64-ready form; a single-query tap gets its row 0 (the only one read)."""
    out = []
    for t in taps:
        q, k = t.q.detach().cpu(), t.k.detach().cpu()
        if q.shape[2] == 1:
            full = torch.zeros(k.shape, dtype=q.dtype)
            full[:, :, :1] = q
            q = full
        out.append((q, k, t.dh ** -0.5))
    return out


@pytest.mark.parametrize("over", [dict(pool="mean"), dict(heads=1, dim_head=64)], ids=["pool-mean", "no-projection"])
def test_vivit_uniform_start_and_dense_last_layers(dvt, device, fx, over):
    """pool='mean': uniform temporal start, dense last temporal layer.  heads=1, dim_head=dim: no output projection, so no
    CLS pruning -- every last layer dense.  Against the restatement on the model's own Q and K, fp32 mode."""
    from dvt_amd import functional as F
    from dvt_amd.rollout import AttentionRollout
    pool = over.get("pool", "cls")
    net = _fixture_model(dvt, fx, torch.float32, **over).to(device).eval()
    clip = torch.from_numpy(fx["clip"]).to(device)
    with torch.no_grad(), F.attention_tap() as taps:
        plain = net(clip)
    depth = int(fx["cfg_depth"])
    kinds = [t.kind for t in taps]
    if "heads" in over:
        assert kinds == ["dense"] * (2 * depth)
    else:
        assert kinds == ["dense"] * (depth - 1) + ["cls"] + ["dense"] * depth
    ro = AttentionRollout(net, residual=RHO)
    r_space, r_time = ro.rows(clip)
    assert torch.equal(ro.outputs, plain)
    ref_s = R.rollout(_layers_of(taps[:depth]), RHO, query=0)
    ref_t = R.rollout(_layers_of(taps[depth:]), RHO, query=None if pool == "mean" else 0)
    es, et = rel_l2(r_space, ref_s), rel_l2(r_time, ref_t)
    print(f"[rollout] ViViT {over}: r_space {es:.2e}, r_time {et:.2e}")
    assert es <= 1e-3 and et <= 1e-3
    assert float((r_time.double().cpu().sum(1) - 1).abs().max()) <= 1e-5


# ---------------------------------------------------------------- FrameTransformer, "vid" mode
class _FixedTokens(torch.nn.Module):
    """Stands for the video encoder: whatever the chunks, the token embeddings are these (the test is about the 14-token stack)."""

    def __init__(self, emb):
        super().__init__()
        self.register_buffer("emb", emb)

    def forward(self, x):
        assert x.shape[0] == self.emb.shape[0]
        return self.emb


def test_frame_transformer_chunks(dvt, device):
    from dvt_amd.models.frame_transformer import FrameTransformer
    from dvt_amd.rollout import AttentionRollout
    B, d = 2, 896
    rng = np.random.default_rng(41)
    emb = torch.from_numpy(rng.standard_normal((B * 14, d))).float()
    net = FrameTransformer(batch_size=B, seq_len=13, cls=1, model="vid", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
                           momentum=0.005, frame_len=2, clip_size=8, encoder_dropout=0.0, compute_dtype=torch.float32,
                           vid_encoder=_FixedTokens(emb))
    with torch.no_grad():
        for name, p in net.distil_transformer.named_parameters():
            if name.endswith("in_proj_weight"):
                p.mul_(3.0)                                               # peaked attention: a wrong order would show
    enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(d, 2, 512, dropout=0.0), 4,
                                      enable_nested_tensor=False).double().eval()
    enc.load_state_dict({k: v.double() for k, v in net.distil_transformer.transformer.state_dict().items()})
    x = emb.double().view(B, 14, d).permute(1, 0, 2) + net.position_encoder.pe[:14].double()
    layers = R.torch_encoder_layers(enc, x)
    assert len(layers) == 4 and layers[0][0].shape == (B, 2, 14, 448)
    ref = R.rollout(layers, RHO, query=0)[:, 1:]
    net = net.to(device).train()
    vid = torch.zeros(B, 13, 2, 3, 8, 8, device=device)
    ro = AttentionRollout(net, residual=RHO)
    chunks = ro.maps(vid)
    assert chunks.shape == (B, 13) and chunks.dtype == torch.float32 and net.training
    assert torch.equal(ro(vid), chunks) and ro.outputs.shape == (B, 19)
    err = rel_l2(chunks, ref)
    print(f"[rollout] FrameTransformer chunks rel {err:.2e}; max/min {float(ref.max() / ref.min()):.1f}")
    assert err <= 1e-3
    assert float(ref.max() / ref.min()) > 1.5


# ---------------------------------------------------------------- state, tap, render
def test_call_leaves_the_model_as_found_and_the_tap_changes_nothing(dvt, device, fx):
    from dvt_amd import functional as F
    from dvt_amd.rollout import AttentionRollout
    net = _fixture_model(dvt, fx, torch.bfloat16).to(device).train()
    net.space_transformer.eval()                                          # a mixed state must come back as it was
    clip = torch.from_numpy(fx["clip"]).to(device)
    flags = [m.training for m in net.modules()]
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ro = AttentionRollout(net)
    mask = ro(clip)
    assert mask.shape == (2, 3, 32, 32) and mask.dtype == torch.float32
    assert flags == [m.training for m in net.modules()] and F._attn_tap is None
    assert all(p.grad is None for p in net.parameters())
    assert all(torch.equal(v, state[k]) for k, v in net.state_dict().items())
    # a forward that raises inside the tap leaves no tap and no eval() behind
    with pytest.raises(ValueError, match="frames"):
        ro(clip[:, :2])
    assert F._attn_tap is None and flags == [m.training for m in net.modules()]
    # the tap only keeps references: outputs with and without it are bit-equal
    net.eval()
    with torch.no_grad():
        plain = net(clip)
        with F.attention_tap() as taps:
            tapped = net(clip)
    assert torch.equal(plain, tapped) and len(taps) == 6
    # render: the call is cam_render of the scaled video map, bit for bit
    r_space, r_time = ro.rows(clip)
    raw, scaled = dvt.ops.rollout_video(r_space, r_time)
    assert torch.equal(mask, dvt.ops.cam_render(scaled.view(2, 3, 4, 4), (3, 32, 32))[0])
    assert torch.equal(ro(clip, scale=False), dvt.ops.cam_render(raw.view(2, 3, 4, 4), (3, 32, 32))[0])
    assert float(mask.min()) >= 0.0 and float(mask.max()) <= 1.0
