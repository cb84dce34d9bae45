"""Class-activation maps on the GPU (csrc/cam.hip, dvt_amd/cam.py, VideoResNet's tap, FrameTransformer.explain) against
the float64 restatement tests/cam_ref.py.  Every bound below is derived from the number formats or is the project's
"2x the restatement's own deviation" protocol; each test prints its figures before it asserts."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import cam_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = 2.0 ** -24                                       # unit round-off of fp32


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


# ---------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("mode", list(DTYPES))
def test_map_exact_on_integers(dvt, device, mode):
    """Integers in [-3, 3], P = 16: every sum and the division by P are exact in fp32, so weights and raw equal the float64
    values bit for bit; scaled is one subtraction, one addition and one division in fp32 (3 roundings of a value <= 1:
    within 2 ulp = 2^-22).  Clip 2 has A >= 0 and G < 0 everywhere: its raw and scaled rows are zero, never NaN."""
    rng = np.random.default_rng(3)
    A = rng.integers(-3, 4, (3, 16, 64)).astype(np.float64)
    G = rng.integers(-3, 4, (3, 16, 64)).astype(np.float64)
    A[2] = rng.integers(0, 4, (16, 64))
    G[2] = -rng.integers(1, 4, (16, 64))
    A, G = torch.from_numpy(A), torch.from_numpy(G)
    dt = DTYPES[mode]
    scaled, raw, w = dvt.ops.cam_map(A.to(dt).to(device), G.to(dt).to(device), "gradcam", want_weights=True, want_raw=True)
    assert dvt.ops.cam_map_launches(16, 64) == 1
    w64, r64, s64 = R.cam(A, G, "gradcam")
    assert torch.equal(w.cpu(), w64.float()) and torch.equal(raw.cpu(), r64.float())
    assert float(r64[:2].max()) > 0
    assert torch.equal(raw[2].cpu(), torch.zeros(16)) and torch.equal(scaled[2].cpu(), torch.zeros(16))
    assert bool(torch.isfinite(scaled).all())
    e = float((scaled.cpu().double() - s64).abs().max())
    print(f"[cam exact/{mode}] scaled max abs {e:.2e} (bound {2.0 ** -22:.2e})")
    assert e <= 2.0 ** -22


# ---------------------------------------------------------------- 2. general shapes
SHAPES = [(2, 2, 3, 3, 512), (2, 3, 6, 6, 256), (1, 1, 7, 5, 64), (5, 1, 1, 1, 128), (1, 12, 24, 24, 64)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, mode):
    """A non-negative with sum_p A >= 1 (a post-ReLU map), G of either sign, rounded to the dtype: (A, G) as float64 [N, P, C]."""
    rng = np.random.default_rng([list(DTYPES).index(mode)] + list(shape))
    N, C = shape[0], shape[-1]
    P = int(np.prod(shape[1:4]))
    A = np.abs(rng.standard_normal((N, P, C))) * (rng.random((N, P, C)) < 0.6)
    A[:, 0, :] += 1.0
    G = 0.05 * rng.standard_normal((N, P, C))
    dt = DTYPES[mode]
    return torch.from_numpy(A).to(dt).double(), torch.from_numpy(G).to(dt).double()


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_general_shapes(dvt, device, shape, mode):
    """Grad-CAM: |raw - ref| <= (P + C + 16) 2^-24 sum_c (sum_p |G| / P) |A| elementwise (P-term and C-term fp32 sums, each
    at most (terms) roundings of the running sum, plus the division, the products and the fused adds).  Grad-CAM++ and
    XGrad-CAM: rel-L2 against float64 within 4x the deviation of the same formulas evaluated by torch on the CPU in float32
    (the summation orders differ), floor 1e-6.  scaled: within 2 ulp of the float64 scaling of the device's own raw row."""
    A, G = _inputs(shape, mode)
    N, P, C = A.shape
    dt = DTYPES[mode]
    Ad, Gd = A.to(dt).to(device), G.to(dt).to(device)
    assert dvt.ops.cam_map_launches(P, C) == (3 if shape == SHAPES[-1] else 1)
    for method in R.METHODS:
        scaled, raw, w = dvt.ops.cam_map(Ad, Gd, method, want_weights=True, want_raw=True)
        w64, r64, _ = R.cam(A, G, method)
        assert bool(torch.isfinite(scaled).all()) and float(r64.max()) > 0
        e_s = float((scaled.cpu().double() - R.scale(raw.cpu().double())).abs().max())
        if method == "gradcam":
            bound = (P + C + 16) * U * ((G.abs().sum(1) / P)[:, None, :] * A.abs()).sum(2)
            excess = float(((raw.cpu().double() - r64).abs() - bound).max())
            print(f"[cam {shape}/{mode}/{method}] raw max abs {float((raw.cpu().double() - r64).abs().max()):.2e}, "
                  f"worst bound excess {excess:.2e}; weights rel {rel_l2(w, w64):.2e}; scaled-vs-own-raw {e_s:.2e}")
            assert excess <= 0
        else:
            _, r32, _ = R.cam(A.float(), G.float(), method)
            yard, err = rel_l2(r32, r64), rel_l2(raw, r64)
            print(f"[cam {shape}/{mode}/{method}] raw rel {err:.2e} (torch CPU fp32: {yard:.2e}); weights rel "
                  f"{rel_l2(w, w64):.2e}; scaled-vs-own-raw {e_s:.2e}")
            assert err <= max(4 * yard, 1e-6)
        assert e_s <= 2.0 ** -22
        # without the optional outputs: the same scaled map
        assert torch.equal(dvt.ops.cam_map(Ad, Gd, method)[0], scaled)


# ---------------------------------------------------------------- 3. repeatability
def test_every_launch_is_repeatable(dvt, device):
    for shape in (SHAPES[1], SHAPES[-1]):
        A, G = _inputs(shape, "bf16")
        Ad, Gd = A.to(torch.bfloat16).to(device), G.to(torch.bfloat16).to(device)
        for method in R.METHODS:
            a = dvt.ops.cam_map(Ad, Gd, method, want_weights=True, want_raw=True)
            b = dvt.ops.cam_map(Ad, Gd, method, want_weights=True, want_raw=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (shape, method)
    rng = np.random.default_rng(9)
    logits = torch.from_numpy(rng.standard_normal((7, 896)).astype(np.float32)).to(device)
    assert torch.equal(dvt.ops.cam_seed(logits), dvt.ops.cam_seed(logits))
    m = torch.from_numpy(rng.random((2, 2, 3, 3)).astype(np.float32)).to(device)
    fr = torch.from_numpy(rng.integers(0, 256, (2, 4, 10, 12, 3), dtype=np.uint8)).to(device)
    a, b = dvt.ops.cam_render(m, (4, 10, 12), frames=fr), dvt.ops.cam_render(m, (4, 10, 12), frames=fr)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- 4. seed
@pytest.mark.parametrize("mode", list(DTYPES))
def test_seed(dvt, device, mode):
    """Argmax with ties to the lowest index (numpy.argmax), explicit categories, mixed -1 entries, K below and above a
    wave, 16-bit logits."""
    dt = DTYPES[mode]
    rng = np.random.default_rng(11)
    for K in (19, 896):
        z = torch.from_numpy(rng.standard_normal((9, K)).astype(np.float32)).to(dt)
        z[0] = 0.25                                               # all equal -> 0
        z[1, 3] = z[1, 7] = 9.0                                   # a tie -> 3
        z[2, K - 1] = 9.0                                         # the last entry
        z[3, 5] = z[3, 5 + 64 if K > 64 else 17] = 9.0            # a tie inside one lane's stride
        z[4, 70 if K > 64 else 12] = z[4, 10] = 9.0               # a tie across lanes, the later lane first in memory order
        z[5] = float("-inf")                                      # nothing to prefer -> 0
        want = np.argmax(z.float().numpy(), axis=1)
        got = dvt.ops.cam_seed(z.to(device))
        assert got.dtype == dt and got.shape == z.shape
        assert np.array_equal(got.float().cpu().numpy(), np.eye(K, dtype=np.float32)[want]), (K, "argmax")
        cat = torch.tensor([2, -1, 0, K - 1, -1, 4, 1, -1, 3], dtype=torch.int32)
        want2 = np.where(cat.numpy() < 0, want, cat.numpy())
        got2 = dvt.ops.cam_seed(z.to(device), cat.to(device))
        assert np.array_equal(got2.float().cpu().numpy(), np.eye(K, dtype=np.float32)[want2]), (K, "categories")
    assert dvt.ops.cam_seed(torch.zeros((0, 19), dtype=dt, device=device)).shape == (0, 19)


# ---------------------------------------------------------------- 5. render
@pytest.mark.parametrize("src,dst", [((2, 3, 3), (12, 48, 48)), ((2, 3, 5), (5, 7, 11)), ((1, 7, 7), (1, 224, 224)),
                                     ((2, 5, 6), (2, 5, 6))], ids=str)
def test_render_upsample(dvt, device, src, dst):
    """Three nested fp32 lerps of values in [0, 1] (weights exact to ~1 ulp of a coordinate below 8): within 2e-6 absolute of
    float64, and of torch's own CUDA interpolate; same size is a bit-equal copy."""
    x = torch.from_numpy(np.random.default_rng(5).random((3,) + src).astype(np.float32))
    mask, over = dvt.ops.cam_render(x.to(device), dst)
    assert over is None and mask.shape == (3,) + dst and mask.dtype == torch.float32
    e = float((mask.cpu().double() - R.interpolate(x, dst)).abs().max())
    own = torch.nn.functional.interpolate(x.to(device)[:, None], size=dst, mode="trilinear", align_corners=False)[:, 0]
    e2 = float((mask - own).abs().max())
    print(f"[cam render {src}->{dst}] vs float64 {e:.2e}, vs torch CUDA {e2:.2e}")
    assert e <= 2e-6 and e2 <= 2e-6
    if src == dst:
        assert torch.equal(mask.cpu(), x)


def _overlay_case(rng):
    """Three 16 x 16 frames: every table entry i / 255 (0 and 1 among them); the breakpoints of the JET ramps and values either
    side; random."""
    m = np.zeros((3, 16, 16), np.float32)
    m[0] = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(16, 16)
    bp = np.array([0.0, 0.125, 0.375, 0.625, 0.875, 1.0], np.float32)
    m[1] = np.resize(np.concatenate([bp, bp - np.float32(1e-3), bp + np.float32(1e-3)]).clip(0, 1), (16, 16))
    m[2] = rng.random((16, 16)).astype(np.float32)
    return m


@pytest.mark.parametrize("use_rgb", [False, True])
@pytest.mark.parametrize("image_weight", [0.5, 0.3])
@pytest.mark.parametrize("kind", ["uint8", "float"])
def test_render_overlay(dvt, device, kind, image_weight, use_rgb):
    """Every byte within +-1 of the restatement (the device blends in fp32 and truncates; a wrong table entry, weight or
    maximum is off by far more)."""
    from dvt_amd import cam
    rng = np.random.default_rng(21)
    m = _overlay_case(rng)
    img = rng.integers(0, 256, (3, 16, 16, 3), dtype=np.uint8)
    if kind == "float":
        img = rng.random((3, 16, 16, 3)).astype(np.float32)
    want = R.overlay(img, m, use_rgb, image_weight).astype(np.int64)
    got = cam.show_cam_on_image(torch.from_numpy(img).to(device), torch.from_numpy(m).to(device), use_rgb=use_rgb,
                                image_weight=image_weight)
    assert got.dtype == torch.uint8 and got.shape == (3, 16, 16, 3)
    d = np.abs(got.cpu().numpy().astype(np.int64) - want)
    print(f"[cam overlay {kind} iw={image_weight} rgb={use_rgb}] max byte difference {d.max()}, bytes off by one {int((d == 1).sum())}")
    assert d.max() <= 1
    assert int(want.max()) == 255 and len(np.unique(want)) > 100
    # mask and overlay from one launch, through the upsample: T' = 1 -> T = 1
    small = torch.from_numpy(rng.random((3, 1, 4, 4)).astype(np.float32)).to(device)
    mask, over = dvt.ops.cam_render(small, (1, 16, 16), frames=torch.from_numpy(img).to(device)[:, None], use_rgb=use_rgb,
                                    image_weight=image_weight)
    want2 = R.overlay(img, mask[:, 0].cpu().numpy(), use_rgb, image_weight).astype(np.int64)
    assert np.abs(over[:, 0].cpu().numpy().astype(np.int64) - want2).max() <= 1


def test_render_overlay_of_a_zero_frame(dvt, device):
    """The frame maximum is 0 only where nothing contributes: an all-black frame, a zero mask and image_weight 1 (at a smaller
    weight JET[0] = (0, 0, 128) is in the blend).  The library divides 0 by 0 there; the device writes zeros."""
    from dvt_amd import cam
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=device)
    img[1] = 200
    out = cam.show_cam_on_image(img, torch.zeros((2, 8, 8), device=device), image_weight=1.0)
    assert torch.equal(out[0], torch.zeros_like(out[0])) and torch.equal(out[1], torch.full_like(out[1], 255))


# ---------------------------------------------------------------- 6. backbone end to end
TARGETS = [5, 700, 33]


@functools.lru_cache(maxsize=None)
def _backbone_case():
    from dvt_amd.models.video_resnet import r2plus1d_18
    rng = np.random.default_rng(17)
    net = r2plus1d_18(num_classes=896, compute_dtype=torch.float32)
    R.fill_backbone(net, rng)
    x = torch.from_numpy(rng.standard_normal((3, 3, 12, 48, 48)).astype(np.float32))
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return state, x


@functools.lru_cache(maxsize=None)
def _backbone_ref(tap, method, kind):
    state, x = _backbone_case()
    dt = {"f64": torch.float64, "f32": torch.float32, "bf16_cast": torch.bfloat16, "bf16_amp": torch.bfloat16}[kind]
    return R.backbone_cam(x, state, tap, TARGETS, method, dt, amp=kind.endswith("amp"))


def _net(device, dtype):
    from dvt_amd.models.video_resnet import r2plus1d_18
    state, x = _backbone_case()
    net = r2plus1d_18(num_classes=896, compute_dtype=dtype)
    net.load_state_dict(state)
    return net.to(device), x.to(device)


@pytest.mark.parametrize("tap,method", [("layer4", "gradcam"), ("layer3", "gradcam"), ("layer3", "gradcam++"),
                                        ("layer4", "xgradcam")])
def test_backbone_maps_match_restatement_fp32(dvt, device, tap, method):
    """fp32 kernels against the restatement in float64, raw and scaled, within 2x the deviation of its own fp32 run (floor
    1e-4); for layer 4 also against the closed form relu(A . W_fc[target]) / P on the module's own tapped A."""
    from dvt_amd import cam
    net, x = _net(device, torch.float32)
    layer = getattr(net, tap)[-1]
    g = cam.CAM_CLASSES[method](net, [layer])
    targets = torch.tensor(TARGETS, dtype=torch.int32, device=device)
    scaled, raw = g.maps(x, targets)
    r64, s64 = _backbone_ref(tap + ".1", method, "f64")
    r32, s32 = _backbone_ref(tap + ".1", method, "f32")
    assert tuple(raw.shape) == tuple(r64.shape) == ((3, 2, 3, 3) if tap == "layer4" else (3, 3, 6, 6))
    e_r, e_s, y_r, y_s = rel_l2(raw, r64), rel_l2(scaled, s64), rel_l2(r32, r64), rel_l2(s32, s64)
    print(f"[cam backbone {tap}/{method}] raw rel {e_r:.2e} (restatement's own fp32 {y_r:.2e}); scaled rel {e_s:.2e} (own {y_s:.2e})")
    assert float(r64.max()) > 0 and all(float(r64[i].max()) > 0 for i in range(3))
    assert e_r <= 2 * y_r + 1e-4 and e_s <= 2 * y_s + 1e-4
    # the library's call: targets as objects, the result upsampled to the clip
    out = g(x, [cam.ClassifierOutputTarget(t) for t in TARGETS])
    assert out.shape == (3, 12, 48, 48) and out.dtype == torch.float32
    assert float((out.cpu().double() - R.interpolate(scaled.cpu(), (12, 48, 48))).abs().max()) <= 2e-6
    assert rel_l2(g.raw(x, targets), dvt.ops.cam_render(raw, (12, 48, 48))[0]) <= 1e-6
    if tap == "layer4" and method == "gradcam":
        net.cam_tap = "layer4.1"
        try:
            net.features(x)
            A = net.cam_tapped[0].detach().double().cpu().view(3, 18, 512)
        finally:
            net.cam_tap = net.cam_tapped = None
        W = net.fc.weight.detach().double().cpu()[TARGETS]
        closed = torch.einsum("npc,nc->np", A, W).clamp_min(0) / 18
        bound = (18 + 512 + 16) * U * torch.einsum("npc,nc->np", A.abs(), W.abs()) / 18
        excess = float(((raw.cpu().double().view(3, 18) - closed).abs() - bound).max())
        print(f"[cam backbone layer4 closed form] worst bound excess {excess:.2e}")
        assert excess <= 0


def test_backbone_maps_bf16(dvt, device):
    """bf16 kernels at layer 4 against the restatement's fp32 run, within 2x the larger of its own autocast and cast-to-bf16
    deviations on the same inputs."""
    from dvt_amd import cam
    net, x = _net(device, torch.bfloat16)
    g = cam.GradCAM(net, [net.layer4[-1]])
    scaled, raw = g.maps(x, torch.tensor(TARGETS, dtype=torch.int32, device=device))
    r32, s32 = _backbone_ref("layer4.1", "gradcam", "f32")
    yr = ys = 0.0
    for kind in ("bf16_cast", "bf16_amp"):
        r, s = _backbone_ref("layer4.1", "gradcam", kind)
        yr, ys = max(yr, rel_l2(r, r32)), max(ys, rel_l2(s, s32))
    e_r, e_s = rel_l2(raw, r32), rel_l2(scaled, s32)
    print(f"[cam backbone layer4/bf16] raw rel {e_r:.2e} (restatement's own bf16 {yr:.2e}); scaled rel {e_s:.2e} (own {ys:.2e})")
    assert e_r <= 2 * yr + 1e-4 and e_s <= 2 * ys + 1e-4


# ---------------------------------------------------------------- 7. nothing else moves
def test_cam_call_leaves_the_model_as_it_found_it(dvt, device):
    from dvt_amd import cam
    net, x = _net(device, torch.float32)
    net.eval()
    net.fc.bias.requires_grad_(False)
    net.layer2[0].conv1[1].weight.requires_grad_(False)
    with torch.no_grad():
        plain = net.features(x)
    net.cam_tap = "layer3.1"
    try:
        tapped = net.features(x)
        assert net.cam_tapped[0].requires_grad and net.cam_tapped[0].is_leaf and net.cam_tapped[1:] == (3, 3, 6, 6)
    finally:
        net.cam_tap = net.cam_tapped = None
    assert torch.equal(plain, tapped.detach())
    flags = {k: p.requires_grad for k, p in net.named_parameters()}
    buffers = {k: b.detach().clone() for k, b in net.named_buffers()}
    for layer in (net.layer3[-1], net.layer4[-1]):
        cam.GradCAM(net, [layer])(x)
        assert all(p.grad is None for p in net.parameters())
        assert flags == {k: p.requires_grad for k, p in net.named_parameters()}
        assert all(torch.equal(b, buffers[k]) for k, b in net.named_buffers())
        assert any(k.endswith("num_batches_tracked") for k in buffers)
        assert net.cam_tap is None and net.cam_tapped is None
    with torch.no_grad():
        assert torch.equal(net.features(x), plain)


# ---------------------------------------------------------------- 8. FrameTransformer.explain
def test_frame_transformer_explain(dvt, device):
    """explain() against an oracle assembled as test_default_frame_transformer_vid_step_matches_oracle assembles its own
    (oracle.clip_path.transformer_base and mlp_head3 behind the encoder), with cam_ref.r2plus1d_tapped as the encoder: raw
    maps of all 4 chunk rows of both samples, fp32 kernels against float64 within 2x the oracle's own fp32 deviation (floor
    1e-4).  A sample's maps do not depend on another sample's category."""
    from oracle import clip_path as O
    from dvt_amd.models.frame_transformer import FrameTransformer
    net = FrameTransformer(batch_size=2, seq_len=3, cls=1, model="vid", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
                           momentum=0.005, frame_len=12, clip_size=48, tokens=4, encoder_dropout=0.0,
                           compute_dtype=torch.float32)
    rng = np.random.default_rng(93)
    with torch.no_grad():
        for name, p in net.named_parameters():
            a = rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if name == "vid_cls":
                a = np.float32(0.5) * a
            elif p.dim() == 5:
                a *= np.float32(np.sqrt(2.0 / (p.shape[1] * p.shape[2] * p.shape[3] * p.shape[4])))
            elif p.dim() == 2:
                a *= np.float32(1.0 / np.sqrt(p.shape[1]))
            elif name.endswith("weight"):
                a = 1 + np.float32(0.1) * a
            else:
                a = np.float32(0.1) * a
            p.copy_(torch.from_numpy(a))
        for name, b in net.named_buffers():
            if name.endswith("running_var"):
                b.copy_(torch.from_numpy(1 + np.float32(0.2) * np.abs(rng.standard_normal(tuple(b.shape)).astype(np.float32))))
    B = 2
    vid = torch.from_numpy(rng.standard_normal((B, 3, 12, 3, 48, 48)).astype(np.float32))
    targets = [4, 11]
    state = {k: v.detach().clone() for k, v in net.state_dict().items() if v.dtype.is_floating_point}

    def oracle(dt):
        P = {k: v.to(dt).clone() for k, v in state.items()}
        cls = P["vid_cls"]
        data = torch.cat((cls.unsqueeze(0).expand(B, *cls.shape), vid.to(dt)), dim=1)
        data = data.reshape(-1, *data.shape[2:]).permute(0, 2, 1, 3, 4)                # [B*4, 3, T, H, W]
        bbP = {k[len("vid_model.backbone."):]: v for k, v in P.items() if k.startswith("vid_model.backbone.")}
        A, emb = R.r2plus1d_tapped(data, bbP, "layer4.1", dt)
        seq = emb.reshape(B, 4, -1).permute(1, 0, 2) + P["position_encoder.pe"][:4]
        logits = O.mlp_head3(O.transformer_base(seq, P, "distil_transformer.", 4, 2)[0], P)
        G = R.one_hot_backward(A, logits, targets)
        _, raw, _ = R.cam(R.channels_last(A.detach()), R.channels_last(G), "gradcam")
        return R.interpolate(raw.double().view(B * 4, 2, 3, 3), (12, 48, 48)).view(B, 4, 12, 48, 48)

    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    yard = rel_l2(r32, r64)
    net = net.to(device).train()
    t = torch.tensor(targets, dtype=torch.int32, device=device)
    raw = net.explain(vid.to(device), t, scale=False)
    assert net.training                                                # the mode it was found in
    assert raw.shape == (2, 4, 12, 48, 48) and raw.dtype == torch.float32
    err = rel_l2(raw, r64)
    print(f"[explain] raw maps rel {err:.2e} (oracle's own fp32: {yard:.2e}); per-row maxima "
          f"{[round(float(v), 6) for v in raw.amax(dim=(2, 3, 4)).reshape(-1)]}")
    assert float(r64.max()) > 0 and err <= 2 * yard + 1e-4
    scaled = net.explain(vid.to(device), t)
    assert scaled.shape == (2, 4, 12, 48, 48) and float(scaled.max()) <= 1.0 + 1e-6 and float(scaled.min()) >= 0.0
    other = net.explain(vid.to(device), torch.tensor([targets[0], 2], dtype=torch.int32, device=device), scale=False)
    assert torch.equal(other[0], raw[0]) and not torch.equal(other[1], raw[1])
    assert all(p.grad is None for p in net.parameters()) and net.vid_model.backbone.cam_tap is None
    net.hparams.model = "frame"
    with pytest.raises(NotImplementedError):
        net.explain(vid.to(device))
