"""Expert embeddings on the MI355X: dvt_conv3d_implicit against CPU float64 F.conv3d, r3d_18 against a CPU torch restatement
with the same weights, ResNet-50 ``embed`` against the imported reference (tests/golden/embed_resnet50.npz), and the
EmbeddingExtractor's keys against the same CPU compositions.  Bounds: rel-L2 1e-5 fp32, 2e-3 fp16, 1e-2 bf16 per
convolution (inputs and weights rounded to the dtype, then float64); whole nets 1e-4 fp32, fixed bounds below otherwise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.embed_fill import fill_resnet50, fill_video_net, resnet50_input
from tests.util import golden, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CONV_TOL = {"fp32": 1e-5, "fp16": 2e-3, "bf16": 1e-2}
NET_TOL = {"fp32": 1e-4, "fp16": 1e-2, "bf16": 4e-2}     # 17 chained convolutions, each rounded to the map dtype


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


# (N, Cin, T, H, W, Cout, k, stride, pad): the r3d_18 layers at reduced T / H / W (the table of DESIGN 4.11), odd shapes
GEOMS = {
    "stem": (1, 3, 4, 30, 30, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3)),
    "layer1": (2, 64, 4, 14, 14, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    "layer2_first": (1, 64, 4, 14, 14, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    "layer2": (1, 128, 4, 7, 7, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    "layer3_first": (1, 128, 4, 14, 14, 256, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    "layer3": (1, 256, 4, 14, 14, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    "layer4_first": (1, 256, 4, 14, 14, 512, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    "layer4_splitk": (1, 512, 2, 7, 7, 512, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    "downsample": (2, 64, 4, 14, 14, 128, (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    "odd": (2, 16, 5, 9, 7, 24, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    "odd_strided": (3, 8, 5, 11, 13, 40, (3, 5, 3), (2, 2, 1), (1, 2, 1)),
}


def _cp(c):
    return (c + 7) // 8 * 8


def _ndhwc(x, cp, dtype, device):
    """[N, C, T, H, W] -> NDHWC [N*T*H*W, cp] (channels past C zero) on the device."""
    N, C, T, H, W = x.shape
    y = torch.zeros(N, T, H, W, cp)
    y[..., :C] = x.permute(0, 2, 3, 4, 1)
    return y.reshape(-1, cp).to(device=device, dtype=dtype)


def _conv_case(dvt, device, name, mode, *, scale=False, shift=False, residual=False, relu=False, seed=0):
    from dvt_amd import ops
    N, Cin, T, H, W, Cout, k, s, p = GEOMS[name]
    dtype = DTYPES[mode]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, T, H, W, generator=g)
    w = torch.randn(Cout, Cin, *k, generator=g) * (2.0 / (Cin * k[0] * k[1] * k[2])) ** 0.5
    xr, wr = x.to(dtype).double(), w.to(dtype).double()
    ref = TF.conv3d(xr, wr, stride=s, padding=p)                      # [N, Cout, To, Ho, Wo]
    To, Ho, Wo = ref.shape[2:]
    ref = ref.permute(0, 2, 3, 4, 1).reshape(-1, Cout)
    sc = (1 + 0.2 * torch.randn(Cout, generator=g)) if scale else None
    sh = 0.3 * torch.randn(Cout, generator=g) if shift else None
    res = torch.randn(ref.shape[0], Cout, generator=g).to(dtype) if residual else None
    if sc is not None:
        ref = ref * sc.double()
    if sh is not None:
        ref = ref + sh.double()
    if res is not None:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    cp = _cp(Cin)
    xd = _ndhwc(x, cp, dtype, device)
    geom = (N, T, H, W)
    K = ops.conv3d_implicit_k(xd, geom, Cout, k, s, p)
    wd = ops.conv3d_weight_pack(w.to(device), cp, K, dtype)
    out = ops.conv3d_implicit(xd, wd, geom, Cout, k, s, p, scale=None if sc is None else sc.to(device),
                              shift=None if sh is None else sh.to(device),
                              residual=None if res is None else res.to(device), relu=relu)
    assert out.shape == (N * To * Ho * Wo, Cout) and out.dtype == dtype
    return out, ref, (xd, wd, geom, Cout, k, s, p, sc, sh, res, relu)


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("name", list(GEOMS))
def test_conv3d_implicit_matches_float64_conv3d(dvt, device, name, mode):
    out, ref, _ = _conv_case(dvt, device, name, mode)
    err = rel_l2(out.double().cpu(), ref)
    print(f"conv3d {name} {mode}: rel L2 {err:.2e}")
    assert err <= CONV_TOL[mode]


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("epi", ["scale_shift", "residual", "relu", "scale_shift_relu", "all"])
@pytest.mark.parametrize("name", ["odd", "layer4_splitk"])
def test_conv3d_implicit_epilogue(dvt, device, name, epi, mode):
    kw = dict(scale="scale" in epi or epi == "all", shift="shift" in epi or epi == "all",
              residual=epi in ("residual", "all"), relu="relu" in epi or epi == "all")
    out, ref, _ = _conv_case(dvt, device, name, mode, seed=1, **kw)
    err = rel_l2(out.double().cpu(), ref)
    assert err <= CONV_TOL[mode], f"{name}/{epi}/{mode}: {err:.2e}"


@pytest.mark.parametrize("name", ["layer1", "layer4_splitk"])
def test_conv3d_implicit_is_bitwise_reproducible(dvt, device, name):
    from dvt_amd import ops
    out, _, (xd, wd, geom, Cout, k, s, p, sc, sh, res, relu) = _conv_case(dvt, device, name, "bf16", shift=True, relu=True)
    again = ops.conv3d_implicit(xd, wd, geom, Cout, k, s, p, shift=sh.to(device), relu=relu)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))


def test_conv3d_split_k_is_taken_for_layer4_at_one_clip(dvt, device):
    from dvt_amd import _lib as L, ops
    import ctypes
    N, Cin, T, H, W, Cout, k, s, p = GEOMS["layer4_splitk"]
    x = torch.zeros(N * T * H * W, Cin, dtype=torch.bfloat16, device=device)
    d = ops.conv3d_desc(x, None, (N, T, H, W), Cout, k, s, p)
    assert L.load().dvt_conv3d_implicit_workspace_bytes(ctypes.byref(d)) > 0
    N, Cin, T, H, W, Cout, k, s, p = GEOMS["layer1"]
    x = torch.zeros(8 * 16 * 56 * 56, Cin, dtype=torch.bfloat16, device=device)
    d = ops.conv3d_desc(x, None, (8, 16, 56, 56), Cout, k, s, p)
    assert L.load().dvt_conv3d_implicit_workspace_bytes(ctypes.byref(d)) == 0


# ---------------------------------------------------------------- r3d_18 against a CPU restatement
def _cpu_r3d_features(net, x):
    """The torchvision r3d_18 forward (eval BatchNorm) in CPU float32 torch, on net's own parameters."""
    def cbr(y, conv, bn, relu=True, res=None):
        y = TF.conv3d(y, conv.weight, stride=conv.stride, padding=conv.padding)
        y = TF.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        if res is not None:
            y = y + res
        return y.clamp_min(0) if relu else y
    with torch.no_grad():
        y = cbr(x, net.stem[0], net.stem[1])
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                out = cbr(y, blk.conv1[0], blk.conv1[1])
                r = y if blk.downsample is None else cbr(y, blk.downsample[0], blk.downsample[1], relu=False)
                y = cbr(out, blk.conv2[0], blk.conv2[1], res=r)
        return y.mean(dim=(2, 3, 4))


@pytest.fixture(scope="module")
def r3d_case():
    from dvt_amd.models.video_resnet import r3d_18
    net = r3d_18(compute_dtype=torch.float32)
    fill_video_net(net, 18)
    net.eval()
    rng = np.random.default_rng(19)
    clips = {"full": torch.from_numpy(rng.standard_normal((2, 3, 16, 112, 112)).astype(np.float32)),
             "odd": torch.from_numpy(rng.standard_normal((1, 3, 5, 64, 48)).astype(np.float32))}
    refs = {k: _cpu_r3d_features(net, v) for k, v in clips.items()}
    return net, clips, refs


@pytest.mark.parametrize("shape,mode", [("full", "fp32"), ("full", "bf16"), ("odd", "fp32"), ("odd", "bf16"),
                                        ("odd", "fp16")])
def test_r3d_18_features_match_cpu_restatement(dvt, device, r3d_case, shape, mode):
    import copy
    net0, clips, refs = r3d_case
    net = copy.deepcopy(net0).to(device)
    net.compute_dtype = DTYPES[mode]
    with torch.no_grad():
        f = net.features(clips[shape].to(device))
    assert f.shape == (clips[shape].shape[0], 512)
    err = rel_l2(f.float().cpu(), refs[shape])
    print(f"r3d_18 {shape} {mode}: rel L2 {err:.2e}")
    assert err <= NET_TOL[mode]


def test_r3d_18_refuses_training_and_grad(dvt, device, r3d_case):
    import copy
    net = copy.deepcopy(r3d_case[0]).to(device)
    x = r3d_case[1]["odd"].to(device)
    net.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        net.features(x)
    net.eval()
    with pytest.raises(RuntimeError, match="inference-only"):
        net.features(x)                       # grad enabled, parameters require grad


def test_conv3d_cache_follows_load_state_dict(dvt, device):
    from dvt_amd.models.video_resnet import r3d_18
    net = r3d_18(compute_dtype=torch.float32)
    fill_video_net(net, 3)
    net = net.to(device).eval()
    x = torch.randn(1, 3, 4, 32, 32, device=device)
    with torch.no_grad():
        a = net.features(x)
        other = r3d_18(compute_dtype=torch.float32)
        fill_video_net(other, 4)
        net.load_state_dict(other.state_dict())
        b = net.features(x)
        ref = _cpu_r3d_features(other.eval(), x.cpu())
    assert rel_l2(b.cpu(), ref) <= NET_TOL["fp32"]
    assert rel_l2(a.cpu(), ref) > 1e-2


# ---------------------------------------------------------------- ResNet-50 embed against the imported reference
@pytest.mark.parametrize("mode", list(DTYPES))
def test_resnet50_embed_matches_reference_golden(dvt, device, mode):
    from dvt_amd.models.custom_resnet import resnet50
    g = golden("embed_resnet50.npz")
    net = resnet50(compute_dtype=DTYPES[mode])
    assert [n for n, _ in net.named_parameters()] == list(g["keys"])
    fill_resnet50(net, int(g["seed"]))
    net = net.to(device).eval()
    x = resnet50_input(int(g["x_seed"]), *g["shape"][[0, 2]])
    with torch.no_grad():
        e = net.embed(x.to(device))
    assert e.shape == (2, 2048)
    err = rel_l2(e.float().cpu(), torch.from_numpy(g["embed"]))
    bound = 1e-4 if mode == "fp32" else max(2 * float(g[f"{mode}:err"]), 5e-3)
    print(f"resnet50 embed {mode}: rel L2 {err:.2e} (bound {bound:.2e})")
    assert err <= bound


# ---------------------------------------------------------------- EmbeddingExtractor
@pytest.fixture(scope="module")
def extractor(dvt, device, r3d_case, tmp_path_factory):
    from dvt_amd.models.pretrained.models import EmbeddingExtractor
    from dvt_amd.models.custom_resnet import resnet50
    d = tmp_path_factory.mktemp("experts")
    r50 = resnet50(compute_dtype=torch.float32)
    fill_resnet50(r50)
    torch.save(r50.state_dict(), d / "r50.pth")
    r50b = resnet50(compute_dtype=torch.float32)
    fill_resnet50(r50b, 77)
    torch.save(r50b.state_dict(), d / "loc.pth")
    torch.save(r3d_case[0].state_dict(), d / "r3d.pth")
    ex = EmbeddingExtractor({"gpu": device.index or 0, "compute_dtype": "fp32", "image_net_weights": str(d / "r50.pth"),
                             "location_net_weights": str(d / "loc.pth"), "video_net_weights": str(d / "r3d.pth")})
    return ex, r50.eval(), r50b.eval(), r3d_case[0]


def _cpu_r50_embed(net, x):
    with torch.no_grad():
        y = TF.relu(TF.batch_norm(TF.conv2d(x, net.conv1.weight, stride=2, padding=3), net.bn1.running_mean,
                                  net.bn1.running_var, net.bn1.weight, net.bn1.bias, False, 0.0, net.bn1.eps))
        y = TF.max_pool2d(y, 3, 2, 1)

        def bn(z, m):
            return TF.batch_norm(z, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                out = TF.relu(bn(TF.conv2d(y, blk.conv1.weight), blk.bn1))
                out = TF.relu(bn(TF.conv2d(out, blk.conv2.weight, stride=blk.conv2.stride, padding=1), blk.bn2))
                out = bn(TF.conv2d(out, blk.conv3.weight), blk.bn3)
                r = y if blk.downsample is None else bn(TF.conv2d(y, blk.downsample[0].weight,
                                                                  stride=blk.downsample[0].stride), blk.downsample[1])
                y = TF.relu(out + r)
        return y.mean(dim=(2, 3))


def test_extractor_image_and_location_keys(dvt, device, extractor):
    ex, r50, r50b, _ = extractor
    rng = np.random.default_rng(5)
    raw = [torch.from_numpy(rng.standard_normal((2, 1, 3, 64, 64)).astype(np.float32)) for _ in range(3)]   # 3 images, b = 2
    for key, net in (("image", r50), ("location", r50b)):
        got = ex.return_expert_for_key(key, raw)
        assert got.shape == (2, 2048) and got.device.type == "cpu" and got.dtype == torch.float32
        ref = torch.stack([_cpu_r50_embed(net, img.squeeze(1)) for img in raw]).mean(dim=0)
        err = rel_l2(got, ref)
        print(f"extractor {key}: rel L2 {err:.2e}")
        assert err <= 1e-4
    one = ex.forward_img(raw[0].squeeze(1))
    assert one.shape == (2, 2048) and one.device.type == "cpu"
    dev = ex.extract_images(raw[0].squeeze(1))
    assert dev.is_cuda and rel_l2(dev.cpu(), one) == 0


def test_extractor_video_key(dvt, device, extractor, r3d_case):
    ex, _, _, net = extractor
    clip = r3d_case[1]["odd"][0]                                        # [3, T, H, W]
    for key in ("video", "motion"):
        got = ex.return_expert_for_key(key, clip)
        assert got.shape == (1, 512) and got.device.type == "cpu" and got.dtype == torch.float32
        assert rel_l2(got, r3d_case[2]["odd"]) <= 1e-4
    assert ex.return_expert_for_key("audio", clip) == []
    v = ex.extract_video(clip.unsqueeze(0))
    assert v.is_cuda and v.shape == (1, 512)
