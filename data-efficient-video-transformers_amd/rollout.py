"""Attention rollout (Abnar & Zuidema, 2020): what a video transformer attends to, read off the attention the model
computes anyway (src/models/vit.py:51-53; nn.MultiheadAttention inside the FrameTransformer's encoder layers).

    from dvt_amd.rollout import AttentionRollout
    ro = AttentionRollout(model, residual=0.5)     # model: ViViT, or FrameTransformer in "vid" mode
    mask = ro(clip)                                # ViViT: f32 [b, T, H, W] on the device, scaled, upsampled
    space, time, video = ro.maps(clip)             # raw: [b, t, h, w], [b, t], [b, t, h, w]
    ro.outputs                                     # the logits of that forward
    overlay = show_cam_on_image(frames, mask)      # cam.py

Per layer A = residual I + (1 - residual) mean_h softmax(scale Q K^T); the rollout of a stack is the row r0^T A_L ... A_1 with
r0 the one-hot of the CLS token where the model reads the CLS row, and the uniform vector where it mean-pools (the temporal
stack of ``ViViT(pool='mean')``).  Only that row is ever formed (csrc/attn_rollout.hip): one eval-mode, no-grad forward of
the model itself under ``functional.attention_tap()``, which keeps references to each layer's q, k and lse (ViViT's last
layers run for the CLS query alone exactly as in any eval forward), then per stack one launch for the last layer
(``ops.rollout_from_probs`` on the folded single-query path, a one-hot ``ops.rollout_step`` otherwise) and one
``ops.rollout_step`` per remaining layer, ``ops.rollout_video`` (time x space, scaled per clip like the class-activation
maps) and ``ops.cam_render``.  No host synchronisation, no torch arithmetic, no N x N tensor.

ViViT: ``space[b, f]`` is the h x w map of frame f's patches under the space stack, ``time[b, f]`` the weight of frame f
under the temporal stack, ``video = time * space``.  On a tubelet model (``ViViT(..., tubelet_size=pt)``) "frame" reads
"tubelet": the maps are ``[b, t / pt, h, w]`` over the temporal tokens, and the rendered volume is still the clip's own
``(t, H, W)`` (the trilinear render upsamples time as it does space).  FrameTransformer ("vid" mode): ``ro.maps(vid)`` and ``ro(vid)`` return
``chunks [B, 13]``, the CLS row over the 4-layer encoder without the CLS entry (14 tokens have nothing to upsample).

Deviations: the heads are fused by their mean only (no max / min fusion), there is no ``discard_ratio``, and the rollout is
defined in eval mode (attention dropout would need its mask in the recompute).  The cross-modal modes of the FrameTransformer
and other models raise NotImplementedError.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as F
from . import ops

Tensor = torch.Tensor

__all__ = ["AttentionRollout"]


def _stack_row(layers, residual: float, uniform: bool = False) -> Tensor:
    """The rollout row of one stack from its taps in execution order -> f32 [S, N]."""
    last = layers[-1]
    if last.kind == "folded":
        r = ops.rollout_from_probs(last.P, last.heads, query=0, residual=residual)
    else:
        start = ops.ROLLOUT_UNIFORM if uniform and last.kind == "dense" else 0
        r = ops.rollout_step(last.q, last.k, last.lse, None, query=start, residual=residual)
    for tap in reversed(layers[:-1]):
        r = ops.rollout_step(tap.q, tap.k, tap.lse, r, residual=residual)
    return r


class AttentionRollout:
    """``AttentionRollout(model, residual=0.5)``; see the module docstring.  A call leaves the model as it found it (the
    training flag of every submodule, gradients, BatchNorm statistics, no tap behind), also when the forward raises."""

    def __init__(self, model: nn.Module, residual: float = 0.5):
        from .models.vit import ViViT
        from .models.frame_transformer import FrameTransformer
        if not 0.0 <= residual <= 1.0:
            raise ValueError(f"residual should be in the range [0, 1]. Got: {residual}")
        if isinstance(model, ViViT):
            self.kind = "vivit"
        elif isinstance(model, FrameTransformer):
            mode = model.hparams.model
            if mode != "vid":
                raise NotImplementedError(f"attention rollout: built for mode 'vid' (the video branch's own encoder), not {mode!r}: "
                                          "the rollout through the cross-modal attention is not defined here")
            self.kind = "frame"
        else:
            raise NotImplementedError(f"attention rollout is built for ViViT and for FrameTransformer in 'vid' mode, not "
                                      f"{type(model).__name__}")
        self.model = model
        self.residual = float(residual)
        self.outputs = None           # the model output of the last call

    def _forward(self, *args):
        """One eval-mode, no-grad forward under the tap -> the taps in execution order."""
        flags = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        try:
            with torch.no_grad(), F.attention_tap() as layers:
                out = self.model(*args)
        finally:
            for m, f in flags:
                m.training = f
        self.outputs = out
        return layers

    def rows(self, clip: Tensor):
        """ViViT: the two rollout rows with their CLS entries, r_space [b t, n + 1] and r_time [b, t + 1], f32."""
        if self.kind != "vivit":
            raise NotImplementedError("rows: the space / time rows of a ViViT; a FrameTransformer has one stack (maps)")
        m = self.model
        layers = self._forward(clip)
        depth = len(m.space_transformer.layers)
        if depth == 0 or len(layers) != depth + len(m.temporal_transformer.layers) or len(layers) == depth:
            raise RuntimeError(f"attention rollout: the forward ran {len(layers)} attention layers; the model has {depth} space "
                               f"and {len(m.temporal_transformer.layers)} temporal layers")
        r_space = _stack_row(layers[:depth], self.residual)                           # [b t, n + 1]
        r_time = _stack_row(layers[depth:], self.residual, uniform=m.pool == "mean")  # [b, t + 1]
        return r_space, r_time

    def _grid(self, clip: Tensor):
        p = self.model.patch_size
        return clip.shape[3] // p, clip.shape[4] // p

    def maps(self, x: Tensor):
        """ViViT: clip [b, t, c, H, W] -> raw (space [b, t, h, w], time [b, t], video [b, t, h, w]), f32 (t / tubelet_size
        temporal tokens in place of t on a tubelet model).
        FrameTransformer: vid [B, 13, ...] -> chunks [B, 13]."""
        if self.kind == "frame":
            layers = self._forward(None, x)
            if not layers:
                raise RuntimeError("attention rollout: the forward ran no attention layer")
            return _stack_row(layers, self.residual)[:, 1:]
        r_space, r_time = self.rows(x)
        b, t = r_time.shape[0], r_time.shape[1] - 1
        h, w = self._grid(x)
        video, _ = ops.rollout_video(r_space, r_time)
        return r_space.view(b, t, -1)[:, :, 1:].reshape(b, t, h, w), r_time[:, 1:], video.view(b, t, h, w)

    def __call__(self, x: Tensor, scale: bool = True, size=None):
        """ViViT: the saliency volume [b, T, H, W] (scaled per clip unless scale=False), upsampled to ``size`` (default: the
        clip's own (t, H, W)).  FrameTransformer: chunks [B, 13]."""
        if self.kind == "frame":
            return self.maps(x)
        r_space, r_time = self.rows(x)
        b, t = r_time.shape[0], r_time.shape[1] - 1
        h, w = self._grid(x)
        raw, scaled = ops.rollout_video(r_space, r_time, want_raw=not scale)
        size = (x.shape[1], x.shape[3], x.shape[4]) if size is None else tuple(size)
        return ops.cam_render((scaled if scale else raw).view(b, t, h, w), size)[0]

    forward = __call__
