"""Class-activation maps of the R(2+1)D video encoder under the names of the ``pytorch_grad_cam`` library, which the
reference imports at src/main.py:20-22 and src/models/frame_transformer.py:14-16 and uses at src/main.py:93-108
(``GradCAM(model, [model.layer4[-1]])``, ``cam(input_tensor=vid)`` on [N, 3, 12, 112, 112] chunks, ``show_cam_on_image``).

    from dvt_amd.cam import GradCAM, GradCAMPlusPlus, XGradCAM, ClassifierOutputTarget, show_cam_on_image

One forward with a tap at the target block (models/video_resnet.py: everything up to the block runs without autograd, its
output becomes a leaf), one backward that stops there, and three launches of csrc/cam.hip: the seed (one-hot at the target
or at the argmax, no host synchronisation), the map (channel weights, ReLU'd weighted sum, per-clip scaling) and the
trilinear upsample.  The result stays on the device.

Deviations from the library: a 3-D map is resized trilinearly (newer versions of the library use a cubic
``scipy.ndimage.zoom``); the JET table comes from its formula, not from OpenCV's table; float frames get no range check on
the device; the overlay is normalised per frame; one target layer (no multi-layer aggregation); a target is a class index
(``ClassifierOutputTarget``), not an arbitrary callable.  ScoreCAM, AblationCAM, EigenCAM and FullGrad need many forwards
or an SVD and are not built: the names exist and raise NotImplementedError.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from . import ops

Tensor = torch.Tensor

__all__ = ["GradCAM", "GradCAMPlusPlus", "XGradCAM", "ClassifierOutputTarget", "show_cam_on_image",
           "ScoreCAM", "AblationCAM", "EigenCAM", "FullGrad"]


class ClassifierOutputTarget:
    """The library's target: the logit of class ``category``."""

    def __init__(self, category: int):
        self.category = int(category)

    def __call__(self, model_output):
        return model_output[..., self.category]


def _find_tap(model: nn.Module, layer: nn.Module):
    """-> (VideoResNet that owns ``layer``, the block's name in it)."""
    from .models.video_resnet import VideoResNet, BasicStem
    for m in model.modules():
        if isinstance(m, VideoResNet):
            for name, sub in m.named_modules():
                if sub is layer:
                    if isinstance(m.stem, BasicStem):
                        raise NotImplementedError("class-activation maps are built for the R(2+1)D encoder; r3d_18 has no tap")
                    if name.count(".") != 1 or not name.startswith("layer"):
                        raise NotImplementedError(f"target layer {name!r}: the tap sits behind a residual block "
                                                  "(layer1[i] .. layer4[i]) of the R(2+1)D encoder")
                    return m, name
    raise NotImplementedError("the target layer is no block of an R(2+1)D VideoResNet inside the model (the 2-D ResNets and "
                              "r3d_18 carry no class-activation tap)")


def _categories(targets, rows: int, device) -> Optional[Tensor]:
    if targets is None:
        return None
    if isinstance(targets, Tensor):
        cat = targets
        if not cat.is_cuda or cat.dtype not in (torch.int32, torch.int64) or cat.dim() != 1:
            raise TypeError("targets: a device int32 / int64 tensor [rows], a list of ClassifierOutputTarget, or None")
        cat = cat if cat.dtype == torch.int32 else cat.to(torch.int32)
    else:
        if not all(isinstance(t, ClassifierOutputTarget) for t in targets):
            raise NotImplementedError("targets: only ClassifierOutputTarget(category) is built")
        cat = torch.tensor([t.category for t in targets], dtype=torch.int32).to(device, non_blocking=True)
    if cat.shape[0] != rows:
        raise ValueError(f"targets: {cat.shape[0]} targets for {rows} rows of model output")
    return cat


class GradCAM:
    """``GradCAM(model, target_layers)``; ``cam(input_tensor, targets=None)`` -> device tensor [N, T, H, W], fp32, one map per
    clip the tapped encoder saw.  ``model``: an R(2+1)D ``VideoResNet`` or any module that runs one (``FrameTransformer``);
    its output rows are the rows of ``targets``.  ``input_tensor``: the model's argument, or a tuple of its positional
    arguments.  ``scale=False`` (or the ``.raw`` method) returns the unscaled maps upsampled: per-clip scaling hides which
    clip matters.  ``size`` (T, H, W) defaults to the clip size read off the last tensor argument ([N, 3, T, H, W], or the
    chunk stack [B, S, T, 3, H, W]).

    The call leaves every parameter's ``.grad`` and ``requires_grad`` flag, the BatchNorm running statistics and the
    encoder's ``cam_tap`` as it found them."""

    method = "gradcam"

    def __init__(self, model: nn.Module, target_layers: Sequence[nn.Module], reshape_transform=None):
        if len(target_layers) != 1:
            raise NotImplementedError("one target layer: multi-layer aggregation is not built")
        if reshape_transform is not None:
            raise NotImplementedError("reshape_transform: the tapped map is the encoder's own channels-last volume")
        self.model = model.eval()
        self.target_layers = list(target_layers)
        self.backbone, self.tap = _find_tap(model, target_layers[0])
        self.outputs = None           # the model output of the last call (the library keeps it under the same name)

    @staticmethod
    def _size(args):
        for a in reversed(args):
            if isinstance(a, Tensor) and a.dim() == 5:
                return tuple(a.shape[2:])
            if isinstance(a, Tensor) and a.dim() == 6:
                return (a.shape[2], a.shape[4], a.shape[5])
        raise ValueError("cam: pass size=(T, H, W); no clip tensor among the arguments to read it from")

    def maps(self, input_tensor, targets=None):
        """The forward, the seed, the truncated backward and the map launch -> (scaled [N, T', H', W'], raw, the same shape)."""
        args = tuple(input_tensor) if isinstance(input_tensor, (tuple, list)) else (input_tensor,)
        if self.model.training:
            raise RuntimeError("cam: the model left eval(); class-activation maps are taken on running statistics")
        bb = self.backbone
        flags = [(p, p.requires_grad) for p in self.model.parameters()]
        for p, _ in flags:
            p.requires_grad_(False)                      # the only leaf of the graph is the tapped map
        bb.cam_tap = self.tap
        try:
            with torch.enable_grad():
                out = self.model(*args)
                if not isinstance(out, Tensor) or out.dim() != 2:
                    raise NotImplementedError("cam: the model must return one [rows, classes] tensor")
                if bb.cam_tapped is None:
                    raise RuntimeError("cam: the model's forward did not run the tapped encoder")
                y, N, T, H, W = bb.cam_tapped
                seed = ops.cam_seed(out, _categories(targets, out.shape[0], out.device))
                (g,) = torch.autograd.grad(out, y, seed)
        finally:
            bb.cam_tap = None
            bb.cam_tapped = None
            for p, f in flags:
                p.requires_grad_(f)
        self.outputs = out.detach()
        C = y.shape[1]
        scaled, raw, _ = ops.cam_map(y.detach().view(N, T * H * W, C), g.view(N, T * H * W, C), self.method, want_raw=True)
        return scaled.view(N, T, H, W), raw.view(N, T, H, W)

    def __call__(self, input_tensor, targets=None, scale: bool = True, size=None):
        args = tuple(input_tensor) if isinstance(input_tensor, (tuple, list)) else (input_tensor,)
        size = self._size(args) if size is None else tuple(size)
        scaled, raw = self.maps(args, targets)
        return ops.cam_render(scaled if scale else raw, size)[0]

    forward = __call__

    def raw(self, input_tensor, targets=None, size=None):
        """The unscaled maps relu(sum_c w A), upsampled."""
        return self(input_tensor, targets, scale=False, size=size)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class GradCAMPlusPlus(GradCAM):
    method = "gradcam++"


class XGradCAM(GradCAM):
    method = "xgradcam"


def _not_built(name: str, why: str):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not built: {why}")
    return type(name, (), {"__init__": __init__, "__doc__": f"Not built: {why}"})


ScoreCAM = _not_built("ScoreCAM", "it needs one forward per channel")
AblationCAM = _not_built("AblationCAM", "it needs one forward per ablated channel")
EigenCAM = _not_built("EigenCAM", "it needs a singular-value decomposition of the activations")
FullGrad = _not_built("FullGrad", "it aggregates the bias gradients of every layer")

CAM_CLASSES = {"gradcam": GradCAM, "gradcam++": GradCAMPlusPlus, "xgradcam": XGradCAM}


def show_cam_on_image(img: Tensor, mask: Tensor, use_rgb: bool = False, image_weight: float = 0.5) -> Tensor:
    """The library's overlay on the device: img [..., H, W, 3] (uint8, or f32 in [0, 1]; frames [H, W, 3], [T, H, W, 3] or
    [N, T, H, W, 3]) and mask [..., H, W] in [0, 1] of the matching shape -> uint8 overlay of img's shape: the JET heat map of
    the mask blended with the image, normalised by the maximum of each frame."""
    if not 0.0 <= image_weight <= 1.0:
        raise ValueError(f"image_weight should be in the range [0, 1]. Got: {image_weight}")
    if img.dim() < 3 or img.shape[-1] != 3 or tuple(mask.shape) != tuple(img.shape[:-1]):
        raise TypeError("show_cam_on_image: img [..., H, W, 3] and mask [..., H, W] of the matching shape")
    H, W = img.shape[-3], img.shape[-2]
    lead = tuple(img.shape[:-3])
    n = 1
    for v in lead:
        n *= v
    m = mask if mask.dtype == torch.float32 else mask.float()
    _, overlay = ops.cam_render(m.reshape(n, 1, H, W), (1, H, W), frames=img.reshape(n, 1, H, W, 3), use_rgb=use_rgb,
                                image_weight=image_weight, want_mask=False)
    return overlay.view(tuple(img.shape))
