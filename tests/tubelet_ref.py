"""CPU restatement of the tubelet embedding (csrc/patchify.hip, functional._PatchEmbed, models.vit), in two independent
formulations:

  * ``gather`` -- reshape / permute: 'b (tau k) c (h p1) (w p2) -> (b tau h w) (k p1 p2 c)';
  * ``gather_conv3d`` / ``embed_conv3d`` -- ``torch.nn.functional.conv3d`` with stride (pt, P, P) over the clip as
    [b, C, t, H, W] and the weight W3[d, c, k, p1, p2] = W[d, ((k P + p1) P + p2) C + c]; with the identity for W the
    convolution IS the gather (products with 0 and 1, sums of one non-zero term: exact in any float type).

Definition, for x [b, t, C, H, W], t % pt == 0, nh = H / P, nw = W / P:
    out[((bi (t/pt) + tau) nh + ph) nw + pw, ((k P + p1) P + p2) C + c] = x[bi, tau pt + k, c, ph P + p1, pw P + p2]
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as TF

# (b, t, C, H, W, P, pt): the gather shapes of the GPU test, with the kernel form each takes
GATHER_SHAPES = [
    (2, 4, 3, 32, 32, 16, 2),      # fast form, 16 rows
    (1, 2, 3, 48, 16, 16, 2),      # 3 rows: a partly filled last wave group
    (1, 6, 3, 16, 24, 8, 3),       # odd pt, vector form
    (2, 4, 1, 8, 12, 4, 4),        # scalar form, pt == t
    # pt = 1, the per-frame gather through the same kernels (ops.patchify is this launch)
    (1, 3, 3, 48, 16, 16, 1),      # fast form, 9 patches of 3 per frame: wave groups straddle frames, the last holds one
    (1, 2, 3, 16, 24, 8, 1),       # vector form
    (2, 2, 1, 8, 12, 4, 1),        # scalar form
]


def gather(x: torch.Tensor, P: int, pt: int) -> torch.Tensor:
    """[b, t, C, H, W] -> [b (t/pt) nh nw, pt P P C] by reshape and permute."""
    b, t, C, H, W = x.shape
    assert t % pt == 0 and H % P == 0 and W % P == 0
    nh, nw = H // P, W // P
    y = x.reshape(b, t // pt, pt, C, nh, P, nw, P)             # b tau k c h p1 w p2
    y = y.permute(0, 1, 4, 6, 2, 5, 7, 3)                      # b tau h w k p1 p2 c
    return y.reshape(b * (t // pt) * nh * nw, pt * P * P * C)


def weight_conv3d(w: torch.Tensor, C: int, P: int, pt: int) -> torch.Tensor:
    """W [d, pt P P C] -> W3 [d, C, pt, P, P]."""
    d = w.shape[0]
    return w.reshape(d, pt, P, P, C).permute(0, 4, 1, 2, 3).contiguous()


def embed_conv3d(x: torch.Tensor, w: torch.Tensor, bias, P: int, pt: int) -> torch.Tensor:
    """[b, t, C, H, W], W [d, pt P P C] -> [b (t/pt) nh nw, d] through conv3d (differentiable)."""
    C = x.shape[2]
    y = TF.conv3d(x.permute(0, 2, 1, 3, 4), weight_conv3d(w, C, P, pt), bias, stride=(pt, P, P))   # [b, d, tau, nh, nw]
    return y.permute(0, 2, 3, 4, 1).reshape(-1, w.shape[0])


def gather_conv3d(x: torch.Tensor, P: int, pt: int) -> torch.Tensor:
    K = pt * P * P * x.shape[2]
    return embed_conv3d(x, torch.eye(K, dtype=x.dtype), None, P, pt)


def per_frame_gather(x: torch.Tensor, P: int) -> torch.Tensor:
    """The per-frame restatement 'b t c (h p1) (w p2) -> (b t h w) (p1 p2 c)', written on its own."""
    b, t, C, H, W = x.shape
    nh, nw = H // P, W // P
    rows = []
    for bi in range(b):
        for f in range(t):
            for ph in range(nh):
                for pw in range(nw):
                    rows.append(x[bi, f, :, ph * P:(ph + 1) * P, pw * P:(pw + 1) * P].permute(1, 2, 0).reshape(-1))
    return torch.stack(rows)


def per_frame_embed(x: torch.Tensor, w2d: torch.Tensor, bias, P: int) -> torch.Tensor:
    y = per_frame_gather(x, P) @ w2d.t()
    return y if bias is None else y + bias


def integer_clip(shape, seed: int, dtype=torch.float64, lo: int = -8, hi: int = 9) -> torch.Tensor:
    """Small integers: every product and sum of the identities stays exact in float64 (and in bf16 for the gather)."""
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, shape)).to(dtype)
