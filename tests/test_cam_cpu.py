"""Class-activation maps, the parts that need no GPU: the restatement (tests/cam_ref.py) pinned from two sides, the C ABI's
declarations and argument checks, and the Python surface."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests import cam_ref as R


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


@pytest.mark.parametrize("src,dst", [((2, 3, 3), (12, 48, 48)), ((2, 3, 5), (5, 7, 11))])
def test_interpolation_restatement_equals_torch(src, dst):
    """The hand-written separable interpolation is torch's trilinear, align_corners=False, in float64 to 1e-12."""
    x = torch.from_numpy(np.random.default_rng(5).random((3,) + src))
    ref = torch.nn.functional.interpolate(x[:, None], size=dst, mode="trilinear", align_corners=False)[:, 0]
    got = R.interpolate(x, dst)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12


def _small_backbone_state(rng, num_classes=896):
    from dvt_amd.models.video_resnet import r2plus1d_18
    net = r2plus1d_18(num_classes=num_classes, compute_dtype=torch.float32)
    R.fill_backbone(net, rng)
    return net


def test_layer4_closed_form_on_the_restatement():
    """Behind the last block there are only the average pool and fc, so Grad-CAM's map has the closed form
    raw = relu(A . W_fc[target]) / P; the restatement's autograd route gives it to round-off."""
    rng = np.random.default_rng(17)
    net = _small_backbone_state(rng)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.from_numpy(rng.standard_normal((3, 3, 12, 48, 48)).astype(np.float32))
    targets = [5, 700, 33]
    A, out = R.r2plus1d_tapped(x, state, "layer4.1", torch.float64)
    assert tuple(A.shape) == (3, 512, 2, 3, 3)
    G = R.one_hot_backward(A, out, targets)
    a = R.channels_last(A.detach())
    _, raw, _ = R.cam(a, R.channels_last(G), "gradcam")
    closed = torch.einsum("npc,nc->np", a, state["fc.weight"].double()[targets]).clamp_min(0) / a.shape[1]
    assert float(raw.max()) > 0
    assert float((raw - closed).norm() / closed.norm()) < 1e-13        # 512-term float64 sums: <= 512 * 2^-53


def test_header_declares_and_lib_binds(dvt):
    L = dvt._lib
    lib = L.load()
    for name in ("dvt_cam_seed", "dvt_cam_map", "dvt_cam_map_launches", "dvt_cam_map_workspace_bytes", "dvt_cam_jet_table",
                 "dvt_cam_render"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert set(L.ENUMS["dvt_cam_method"]) == {"DVT_CAM_GRADCAM", "DVT_CAM_GRADCAMPP", "DVT_CAM_XGRADCAM"}
    assert L.ABI_VERSION == 5
    # the switch-over between the two forms, as the header states it: layers 4 and 3 of the reference default are one launch
    assert lib.dvt_cam_map_launches(2 * 7 * 7, 512) == 1 and lib.dvt_cam_map_launches(3 * 14 * 14, 256) == 1
    assert lib.dvt_cam_map_launches(12 * 56 * 56, 64) == 3 and lib.dvt_cam_map_launches(12 * 24 * 24, 64) == 3
    assert lib.dvt_cam_map_launches(L.MACROS["DVT_CAM_FUSED_MAX_P"], 64) == 1
    assert lib.dvt_cam_map_launches(L.MACROS["DVT_CAM_FUSED_MAX_P"] + 1, 8) == 3
    assert lib.dvt_cam_map_workspace_bytes(28, 98, 512) == 0 and lib.dvt_cam_map_workspace_bytes(1, 12 * 24 * 24, 64) > 0
    jet = np.zeros((256, 3), np.uint8)
    assert lib.dvt_cam_jet_table(jet.ctypes.data, jet.size) == 0
    assert np.array_equal(jet, R.jet_table())
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0) and tuple(jet[128])[1] == 255


def test_entry_points_refuse_bad_arguments_without_a_gpu(dvt):
    """Null pointers, C % 8 != 0 and an unknown method come back as DVT_ERR_BAD_ARG with a message, before any launch; N == 0
    is DVT_OK and launches nothing."""
    L = dvt._lib
    lib = L.load()
    bad, unsupported = L.ENUMS["dvt_status"]["DVT_ERR_BAD_ARG"], L.ENUMS["dvt_status"]["DVT_ERR_UNSUPPORTED"]
    buf = (C.c_float * 72)()                         # a host buffer: a non-null address no call below gets as far as using
    p = (C.addressof(buf) + 15) & ~15
    gc = L.ENUMS["dvt_cam_method"]["DVT_CAM_GRADCAM"]

    def msg():
        return lib.dvt_last_error().decode()

    assert lib.dvt_cam_seed(None, None, p, 2, 19, L.F32, None) == bad and "null" in msg()
    assert lib.dvt_cam_seed(p, None, None, 2, 19, L.F32, None) == bad
    assert lib.dvt_cam_seed(p, None, p, 2, 0, L.F32, None) == bad
    assert lib.dvt_cam_seed(p, None, p, 2, 19, 7, None) == bad and "dtype" in msg()
    assert lib.dvt_cam_seed(None, None, None, 0, 19, L.F32, None) == 0

    assert lib.dvt_cam_map(None, p, 1, 4, 8, L.F32, gc, None, None, p, None, 0, None) == bad and "null" in msg()
    assert lib.dvt_cam_map(p, p, 1, 4, 8, L.F32, gc, None, None, None, None, 0, None) == bad
    assert lib.dvt_cam_map(p, p, 1, 4, 12, L.F32, gc, None, None, p, None, 0, None) == bad and "multiple of 8" in msg()
    assert lib.dvt_cam_map(p, p, 1, 4, 8, L.F32, 3, None, None, p, None, 0, None) == bad and "method" in msg()
    assert lib.dvt_cam_map(p, p, 1, 4, 8, L.F32, -1, None, None, p, None, 0, None) == bad
    assert lib.dvt_cam_map(p, p, 1, 12 * 24 * 24, 64, L.F32, gc, None, None, p, None, 0, None) == bad and "workspace" in msg()
    assert lib.dvt_cam_map(p, p, 1, 4, L.MACROS["DVT_CAM_MAX_C"] + 8, L.F32, gc, None, None, p, None, 0, None) == unsupported
    assert lib.dvt_cam_map(None, None, 0, 4, 8, L.F32, gc, None, None, None, None, 0, None) == 0

    assert lib.dvt_cam_render(None, 1, 1, 2, 2, 1, 4, 4, p, None, 0, None, None, 0.5, 0, None) == bad and "null" in msg()
    assert lib.dvt_cam_render(p, 1, 1, 2, 2, 1, 4, 4, None, None, 0, None, None, 0.5, 0, None) == bad
    assert lib.dvt_cam_render(p, 1, 1, 2, 2, 1, 4, 4, None, p, 0, None, p, 0.5, 0, None) == bad and "jet" in msg()
    assert lib.dvt_cam_render(p, 1, 1, 2, 2, 1, 4, 0, p, None, 0, None, None, 0.5, 0, None) == bad
    assert lib.dvt_cam_render(p, 1, 1, 2, 2, 1, 4, 4, p, None, 0, None, None, 1.5, 0, None) == bad and "image_weight" in msg()
    assert lib.dvt_cam_render(None, 0, 1, 2, 2, 1, 4, 4, None, None, 0, None, None, 0.5, 0, None) == 0
    assert lib.dvt_cam_jet_table(None, 768) == bad and lib.dvt_cam_jet_table(p, 100) == bad


def test_python_surface(dvt):
    from dvt_amd import cam, ops, functional as F
    from dvt_amd.models.video_resnet import r2plus1d_18, r3d_18
    from dvt_amd.models.frame_transformer import FrameTransformer
    for name in ("GradCAM", "GradCAMPlusPlus", "XGradCAM", "ClassifierOutputTarget", "show_cam_on_image"):
        assert hasattr(cam, name)
    assert set(ops.CAM_METHODS) == set(R.METHODS)
    assert F.cam_map is ops.cam_map and F.cam_seed is ops.cam_seed and F.cam_render is ops.cam_render
    net = r2plus1d_18(num_classes=19, compute_dtype=torch.float32).train()
    for name in ("ScoreCAM", "AblationCAM", "EigenCAM", "FullGrad"):
        with pytest.raises(NotImplementedError):
            getattr(cam, name)(net, [net.layer4[-1]])
    with pytest.raises(NotImplementedError):
        cam.GradCAM(net, [net.layer4[-1], net.layer3[-1]])
    assert net.training                                   # (refused before the model was touched)
    g = cam.GradCAMPlusPlus(net, [net.layer3[-1]])
    assert not net.training and g.tap == "layer3.1" and g.backbone is net and g.method == "gradcam++"
    assert cam.XGradCAM.method == "xgradcam" and cam.GradCAM.method == "gradcam"
    assert net.cam_tap is None and "cam_tap" not in net.state_dict() and not any("cam" in k for k in net.state_dict())
    with pytest.raises(NotImplementedError):
        cam.GradCAM(net, [net.layer4[-1].conv1])          # not a block's output
    r3d = r3d_18(num_classes=19)
    with pytest.raises(NotImplementedError):
        cam.GradCAM(r3d, [r3d.layer4[-1]])
    r3d.cam_tap = "layer4.1"
    with pytest.raises(NotImplementedError):
        r3d.eval().features(torch.zeros(1, 3, 4, 16, 16))
    with pytest.raises(NotImplementedError):
        cam.GradCAM(torch.nn.Linear(4, 4), [torch.nn.ReLU()])
    assert cam.ClassifierOutputTarget(3)(torch.arange(5.0)) == 3.0
    assert callable(FrameTransformer.explain)
    with pytest.raises(ValueError):
        ops.cam_map(torch.zeros(1, 2, 8), torch.zeros(1, 2, 8), "scorecam")
