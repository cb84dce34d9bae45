"""CPU-side checks of the expert-embedding extractor (the reference's src/models/pretrained/models.py): module trees and
state-dict keys of r3d_18 and the unchanged R(2+1)D-18, the new C ABI symbols, and EmbeddingExtractor's configuration and
weight loading (built on the CPU; no forward pass)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvt_conv3d_implicit_supported", "dvt_conv3d_implicit_k", "dvt_conv3d_implicit_workspace_bytes",
               "dvt_conv3d_implicit", "dvt_conv3d_weight_pack", "dvt_bn_fold"]
R3D18_PARAMS_400 = 33_371_472          # torchvision.models.video.r3d_18(num_classes=400)


def _torchvision_r3d18_keys():
    """State-dict keys of torchvision's r3d_18: stem.{0,1}, layerL.B.conv{1,2}.{0,1}, layerL.0.downsample.{0,1}, fc."""
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    keys = ["stem.0.weight"] + [f"stem.1.{s}" for s in bn]
    for L in range(1, 5):
        for B in range(2):
            for c in (1, 2):
                keys += [f"layer{L}.{B}.conv{c}.0.weight"] + [f"layer{L}.{B}.conv{c}.1.{s}" for s in bn]
            if B == 0 and L > 1:
                keys += [f"layer{L}.0.downsample.0.weight"] + [f"layer{L}.0.downsample.1.{s}" for s in bn]
    return keys + ["fc.weight", "fc.bias"]


def _r2plus1d_keys():
    """R(2+1)D-18 keys as the tree had them before r3d_18 was added (torchvision's r2plus1d_18)."""
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    keys = ["stem.0.weight"] + [f"stem.1.{s}" for s in bn] + ["stem.3.weight"] + [f"stem.4.{s}" for s in bn]
    for L in range(1, 5):
        for B in range(2):
            for c in (1, 2):
                keys += [f"layer{L}.{B}.conv{c}.0.0.weight"] + [f"layer{L}.{B}.conv{c}.0.1.{s}" for s in bn]
                keys += [f"layer{L}.{B}.conv{c}.0.3.weight"] + [f"layer{L}.{B}.conv{c}.1.{s}" for s in bn]
            if B == 0 and L > 1:
                keys += [f"layer{L}.0.downsample.0.weight"] + [f"layer{L}.0.downsample.1.{s}" for s in bn]
    return keys + ["fc.weight", "fc.bias"]


def test_pretrained_models_module_imports():
    from dvt_amd.models.pretrained import models
    assert models.EmbeddingExtractor and models.Identity
    for name in ("init_models", "forward_img", "forward_location", "forward_video", "forward_depth", "forward_audio",
                 "depth_network_pool", "return_expert_for_key", "return_expert_for_key_pretrained", "extract_images",
                 "extract_video"):
        assert callable(getattr(models.EmbeddingExtractor, name)), name


def test_r3d_18_tree_matches_torchvision():
    from dvt_amd.models.video_resnet import r3d_18, Conv3DSimple, BasicStem
    m = r3d_18()
    assert list(m.state_dict()) == _torchvision_r3d18_keys()
    assert sum(p.numel() for p in m.parameters()) == R3D18_PARAMS_400
    assert isinstance(m.stem, BasicStem) and isinstance(m.layer1[0].conv1[0], Conv3DSimple)
    assert tuple(m.stem[0].kernel_size) == (3, 7, 7) and tuple(m.stem[0].stride) == (1, 2, 2)
    assert tuple(m.layer2[0].downsample[0].stride) == (2, 2, 2)
    with pytest.raises(RuntimeError):
        r3d_18(pretrained=True)


def test_r2plus1d_default_tree_is_unchanged():
    from dvt_amd.models.video_resnet import r2plus1d_18, VideoResNet
    assert list(r2plus1d_18().state_dict()) == _r2plus1d_keys()
    assert list(VideoResNet().state_dict()) == _r2plus1d_keys()


def test_r3d_18_training_mode_is_refused():
    from dvt_amd.models.video_resnet import r3d_18
    with pytest.raises(NotImplementedError, match="inference-only"):
        r3d_18().train().features(torch.zeros(1, 3, 4, 32, 32))


def test_new_symbols_in_header_signatures_and_library():
    import dvt_amd
    from dvt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvt_hip.h")).read()
    tool = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    nm = subprocess.run([tool, "-D", "--defined-only", dvt_amd._lib.LIB_PATH], check=True, capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
        assert s in exported, s
    assert "typedef struct dvt_conv3d_desc" in hdr
    assert _lib.load().dvt_version() == _lib.ABI_VERSION == 5


def test_conv3d_entry_points_validate_before_any_hip_call():
    import ctypes
    from dvt_amd import _lib
    lib = _lib.load()
    d = _lib.Conv3dDesc()
    d.N, d.T, d.H, d.W, d.C, d.Cout = 1, 16, 112, 112, 8, 64
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = 3, 7, 7, 1, 2, 2, 1, 3, 3
    d.dtype = _lib.BF16
    assert lib.dvt_conv3d_implicit_supported(ctypes.byref(d)) == 1
    assert lib.dvt_conv3d_implicit_k(ctypes.byref(d)) == 3 * 7 * 7 * 8 + 8      # 1176 rounded up to the 32-wide k-tile
    assert lib.dvt_conv3d_implicit(ctypes.byref(d), None) == -1                  # null x / w / y
    d.C = 3
    assert lib.dvt_conv3d_implicit_supported(ctypes.byref(d)) == 0
    assert lib.dvt_conv3d_implicit_k(ctypes.byref(d)) == -1
    d.C, d.dtype = 8, 7
    assert lib.dvt_conv3d_implicit(ctypes.byref(d), None) == -2
    assert lib.dvt_conv3d_implicit(None, None) == -1
    assert lib.dvt_conv3d_weight_pack(None, None, 1, 64, 3, 3, 7, 7, 8, 1184, None) == -1
    assert lib.dvt_bn_fold(None, None, None, None, 1e-5, None, None, 64, None) == -1


class _View:
    """confuse-style view: config["gpu"].get(int); .get() of a key that is not set raises NotFoundError."""

    class NotFoundError(Exception):
        pass

    def __init__(self, data, key=None):
        self.data, self.key = data, key

    def __getitem__(self, key):
        return _View(self.data, key)

    def get(self, typ=None):
        if self.key not in self.data:
            raise _View.NotFoundError(self.key)
        v = self.data[self.key]
        return typ(v) if typ is not None else v


def test_extractor_config_forms_weights_and_warning(tmp_path, capsys):
    from dvt_amd.models.pretrained.models import EmbeddingExtractor, Identity
    from dvt_amd.models.video_resnet import r3d_18
    src = r3d_18()
    with torch.no_grad():
        for p in src.parameters():
            p.uniform_(-1, 1)
    sd = src.state_dict()
    assert any(k.startswith("fc.") for k in sd)
    path = tmp_path / "r3d.pth"
    torch.save(sd, path)

    ex = EmbeddingExtractor({"gpu": 0, "video_net_weights": str(path), "compute_dtype": "fp32"})
    err = capsys.readouterr().err
    assert "image_net" in err and "location_net" in err and "video_net" not in err.replace("video_net_weights", "")
    assert ex.device == torch.device("cuda", 0) and ex.compute_dtype == torch.float32
    assert isinstance(ex.video_net.fc, Identity) and isinstance(ex.image_net.fc, Identity)
    got = ex.video_net.state_dict()
    assert not any(k.startswith("fc.") for k in got)
    assert torch.equal(got["layer4.1.conv2.0.weight"], sd["layer4.1.conv2.0.weight"])

    ex2 = EmbeddingExtractor(_View({"gpu": 1}))
    assert ex2.device == torch.device("cuda", 1) and ex2.compute_dtype == torch.bfloat16
    assert ex2.image_net.compute_dtype == torch.bfloat16
    # seeded random init: two extractors without files agree
    ex3 = EmbeddingExtractor({"gpu": 0})
    assert torch.equal(ex2.image_net.conv1.weight, ex3.image_net.conv1.weight)
    assert torch.equal(ex2.video_net.stem[0].weight, ex3.video_net.stem[0].weight)
    assert not torch.equal(ex2.image_net.conv1.weight, ex2.location_net.conv1.weight)


def test_extractor_refusals_and_host_side_pretrained_reshape():
    from dvt_amd.models.pretrained.models import EmbeddingExtractor
    ex = EmbeddingExtractor({"gpu": 0})
    for fn in (ex.forward_depth, ex.forward_audio, ex.depth_network_pool):
        with pytest.raises(NotImplementedError):
            fn(torch.zeros(1))
    raw = [torch.randn(1, 2048) for _ in range(4)]
    out = ex.return_expert_for_key_pretrained("image", raw)
    assert out.shape == (2048,) or out.shape == (1, 2048)
    assert torch.allclose(out.reshape(-1), torch.stack(raw).mean(0).reshape(-1), atol=1e-6)
    v = ex.return_expert_for_key_pretrained("video", [torch.randn(512)])
    assert v.shape == (1, 512)
    assert ex.return_expert_for_key("audio", torch.zeros(1)) == []


def test_pretrained_resnets_refuse_download():
    from dvt_amd.models.custom_resnet import resnet50
    with pytest.raises(RuntimeError):
        resnet50(pretrained=True)
    assert hasattr(resnet50(), "embed")
