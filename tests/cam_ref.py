"""Float64 restatement of the class-activation maps (TEST INFRASTRUCTURE; the device code is csrc/cam.hip): the three
weight rules, the map and its scaling, a hand-written separable interpolation, the JET table and the overlay, and the
R(2+1)D loop of oracle/cnn_path.py with one block's output made a leaf.  Written from the formulas of the issue text, which
are the published ones (Grad-CAM, Grad-CAM++, XGrad-CAM; ``scale_cam_image`` and ``show_cam_on_image`` of the
pytorch_grad_cam library); torch is used for storage, convolutions and autograd only."""
from __future__ import annotations

import numpy as np
import torch

METHODS = ("gradcam", "gradcam++", "xgradcam")


# ---------------------------------------------------------------- weights, map, scaling: A, G [N, P, C]
def weights(A: torch.Tensor, G: torch.Tensor, method: str) -> torch.Tensor:
    """-> w [N, C] in the dtype of A (float64 for the truth, float32 for the yardstick)."""
    P = A.shape[1]
    if method == "gradcam":
        return G.sum(1) / P
    if method == "xgradcam":
        return (G * A).sum(1) / (A.sum(1) + 1e-7)
    if method == "gradcam++":
        S = A.sum(1, keepdim=True)
        g2 = G * G
        a = g2 / (2 * g2 + S * g2 * G + 1e-6)
        a = torch.where(G != 0, a, torch.zeros_like(a))
        return (G.clamp_min(0) * a).sum(1)
    raise ValueError(method)


def raw_map(A: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """raw[n, p] = max(sum_c w[n, c] A[n, p, c], 0)."""
    return (A * w[:, None, :]).sum(2).clamp_min(0)


def scale(raw: torch.Tensor) -> torch.Tensor:
    """scale_cam_image per row: (raw - min) / (1e-7 + max(raw - min))."""
    r = raw - raw.min(1, keepdim=True).values
    return r / (1e-7 + r.max(1, keepdim=True).values)


def cam(A: torch.Tensor, G: torch.Tensor, method: str):
    """-> (weights, raw, scaled) of A, G [N, P, C] in their own dtype."""
    w = weights(A, G, method)
    r = raw_map(A, w)
    return w, r, scale(r)


def channels_last(t: torch.Tensor) -> torch.Tensor:
    """[N, C, T, H, W] -> [N, T*H*W, C]."""
    N, C = t.shape[:2]
    return t.permute(0, 2, 3, 4, 1).reshape(N, -1, C)


# ---------------------------------------------------------------- interpolation
def _axis(I: int, O: int):
    """Taps and weights of one axis: src = (o + 0.5) I / O - 0.5 clamped to [0, I - 1]."""
    src = np.clip((np.arange(O, dtype=np.float64) + 0.5) * I / O - 0.5, 0.0, I - 1.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, I - 1)
    return i0, i1, src - i0


def interpolate(x: torch.Tensor, size) -> torch.Tensor:
    """Separable linear interpolation with half-pixel centres of the last three axes of x [N, T', H', W'] to size = (T, H, W),
    in float64."""
    y = x.double()
    for ax, O in zip((1, 2, 3), size):
        i0, i1, l1 = _axis(y.shape[ax], int(O))
        shape = [1, 1, 1, 1]
        shape[ax] = -1
        l1 = torch.from_numpy(l1).reshape(shape)
        y = y.index_select(ax, torch.from_numpy(i0)) * (1 - l1) + y.index_select(ax, torch.from_numpy(i1)) * l1
    return y


# ---------------------------------------------------------------- overlay
def jet_table() -> np.ndarray:
    """[256, 3] uint8, RGB: x = i / 255; r, g, b = clamp(1.5 - |4x - 3|), clamp(1.5 - |4x - 2|), clamp(1.5 - |4x - 1|);
    entries floor(255 v + 0.5)."""
    x = np.arange(256, dtype=np.float64) / 255.0
    rgb = np.stack([1.5 - np.abs(4 * x - 3), 1.5 - np.abs(4 * x - 2), 1.5 - np.abs(4 * x - 1)], axis=1)
    return np.floor(255.0 * np.clip(rgb, 0.0, 1.0) + 0.5).astype(np.uint8)


def overlay(img: np.ndarray, mask: np.ndarray, use_rgb: bool = False, image_weight: float = 0.5) -> np.ndarray:
    """show_cam_on_image per frame: img [F, H, W, 3] (uint8, or float in [0, 1]), mask float32 [F, H, W] -> uint8 [F, H, W, 3].
    The table index is (int)(255 mask) in float32, as the library forms it (np.uint8(255 * mask) on a float32 mask); the rest
    is float64."""
    idx = np.clip((np.float32(255.0) * mask.astype(np.float32)).astype(np.int64), 0, 255)
    table = jet_table().astype(np.float64) / 255.0
    heat = table[idx]                                            # [F, H, W, 3] RGB
    if not use_rgb:
        heat = heat[..., ::-1]
    pic = img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)
    iw = float(np.float32(image_weight))
    blend = (1.0 - iw) * heat + iw * pic
    mx = blend.reshape(blend.shape[0], -1).max(1)[:, None, None, None]
    out = np.where(mx > 0, 255.0 * blend / np.where(mx > 0, mx, 1.0), 0.0)
    return out.astype(np.uint8)


# ---------------------------------------------------------------- the tapped encoder
def fill_backbone(net, rng):
    """Weights from a numpy stream (He-scaled convolutions, 0.02 n matrices, 1 + 0.1 n scales, 0.1 n shifts and running
    means); running variances 1 + 0.2 |n|."""
    with torch.no_grad():
        for name, p in net.named_parameters():
            a = rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if p.dim() == 5:
                a *= np.float32(np.sqrt(2.0 / (p.shape[1] * p.shape[2] * p.shape[3] * p.shape[4])))
            elif p.dim() == 2:
                a *= np.float32(0.02)
            elif name.endswith("weight"):
                a = 1 + np.float32(0.1) * a
            else:
                a = np.float32(0.1) * a
            p.copy_(torch.from_numpy(a))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.from_numpy(np.float32(0.1) * rng.standard_normal(tuple(b.shape)).astype(np.float32)))
            elif name.endswith("running_var"):
                b.copy_(torch.from_numpy(1 + np.float32(0.2) * np.abs(rng.standard_normal(tuple(b.shape)).astype(np.float32))))


def r2plus1d_tapped(x: torch.Tensor, P: dict, tap: str, dtype: torch.dtype, amp: bool = False, layers=(2, 2, 2, 2)):
    """The R(2+1)D loop of oracle.cnn_path.r2plus1d_features (its _conv2plus1d / _bn3 helpers), eval mode, with the output of
    block ``tap`` ("layer4.1") made a leaf, and ``fc`` applied on the pooled features: -> (A leaf [N, C, T', H', W'],
    outputs [N, K]).  P: the backbone's state dict (fc as ``fc.weight`` or ``fc.0.weight``).  dtype: the dtype everything is
    cast to, or with amp=True the autocast dtype over fp32 weights."""
    from oracle import cnn_path as C
    import torch.nn.functional as TF
    cast = (lambda t: t) if amp else (lambda t: t.to(dtype))
    P = {k: (cast(v) if v.dtype.is_floating_point else v) for k, v in P.items()}
    fc = "fc.0." if "fc.0.weight" in P else "fc."

    def run():
        h = TF.conv3d(cast(x), P["stem.0.weight"], None, (1, 2, 2), (0, 3, 3))
        h = torch.relu(C._bn3(h, P, "stem.1.", False))
        h = TF.conv3d(h, P["stem.3.weight"], None, 1, (1, 0, 0))
        h = torch.relu(C._bn3(h, P, "stem.4.", False))
        A = None
        for li, nb in enumerate(layers):
            for b in range(nb):
                pre = f"layer{li + 1}.{b}."
                stride = 2 if (li > 0 and b == 0) else 1
                with torch.set_grad_enabled(A is not None):
                    out = C._conv2plus1d(h, P, pre + "conv1.0.", stride, False)
                    out = torch.relu(C._bn3(out, P, pre + "conv1.1.", False))
                    out = C._conv2plus1d(out, P, pre + "conv2.0.", 1, False)
                    out = C._bn3(out, P, pre + "conv2.1.", False)
                    res = h
                    if pre + "downsample.0.weight" in P:
                        res = TF.conv3d(h, P[pre + "downsample.0.weight"], None, stride)
                        res = C._bn3(res, P, pre + "downsample.1.", False)
                    h = torch.relu(out + res)
                if pre[:-1] == tap:
                    A = h = h.detach().requires_grad_()
        if A is None:
            raise ValueError(tap)
        with torch.enable_grad():
            feats = h.mean(dim=(2, 3, 4))
            return A, TF.linear(feats, P[fc + "weight"], P[fc + "bias"])

    if amp:
        with torch.autocast("cpu", dtype=dtype):
            return run()
    return run()


def one_hot_backward(A: torch.Tensor, outputs: torch.Tensor, targets) -> torch.Tensor:
    """d(sum_b outputs[b, targets[b]]) / dA."""
    seed = torch.zeros_like(outputs)
    seed[torch.arange(outputs.shape[0]), torch.as_tensor(targets)] = 1
    (g,) = torch.autograd.grad(outputs, A, seed)
    return g


def backbone_cam(x, P, tap, targets, method, dtype, amp=False):
    """-> (raw, scaled) [N, T', H', W'] in float64 of the restatement run in ``dtype``: the encoder, the backward and the map
    arithmetic all in that dtype (autocast: the map arithmetic in fp32), as a user of the library would run them."""
    A, out = r2plus1d_tapped(x, P, tap, dtype, amp)
    G = one_hot_backward(A, out, targets)
    N, _, T, H, W = A.shape
    mdt = torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype
    _, r, s = cam(channels_last(A.detach()).to(mdt), channels_last(G).to(mdt), method)
    return r.double().view(N, T, H, W), s.double().view(N, T, H, W)
