"""Masked-autoencoder pre-training of the ViViT's space stack (MAE / MAE-ST / VideoMAE; the reference has no
self-supervised clip model) on the kernels of csrc/patch_dropout.hip and csrc/mae.hip.

A clip ``[b, t, C, H, W]`` is S = b * t' sequences (t' = t / tubelet_size temporal tokens) of n patch positions.  Every
forward masks: a sequence keeps k = n - floor(mask_ratio * n) positions (``"tube"``: the same in every temporal token of a
clip, VideoMAE's tube masking; ``"frame"``: drawn per temporal token), the encoder runs on those k tokens plus its CLS row, a
light decoder sees all n positions -- the encoded rows where a position was kept, a learned mask token elsewhere -- and the
loss is the mean squared error between its prediction and the pixels of the n - k dropped patches, per-patch normalised under
``norm_pix_loss``.  The decoder attends within one temporal token's n positions, as the space stack does; with
``tubelet_size = pt`` a token and its target span pt frames.

Limits.  Pre-training covers the encoder's patch embedding, positional table, space token and space stack (with its final
norm).  The encoder's temporal stack, ``temporal_token`` and ``mlp_head`` are not part of this forward: they get no gradient
(``grad is None``; under ``dp.FlatParameters`` their gradient views stay unwritten, i.e. zero, as the optimizers expect of
unused parameters).  The encoder's own ``patch_dropout`` and ``drop_path`` settings are ignored here: the mask ratio decides
what is kept, and every residual branch runs on every sequence.  There is no CPU path.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .. import functional as F
from .vit import Transformer, ViViT


class MaskedClipAutoencoder(nn.Module):
    """``forward(x[b, t, c, H, W], keep=None) -> (loss, pred [S, n, pt*P*P*C], slot [S, n])``.

    Parameters: ``encoder.*`` (the ViViT's own keys), ``decoder_embed.{weight,bias}`` (dim -> decoder_dim), ``mask_token
    [1, 1, decoder_dim]``, ``decoder_pos_embedding [1, t', n, decoder_dim]``, ``decoder`` (the project's ``Transformer``,
    final norm included) and ``decoder_pred.{weight,bias}`` (decoder_dim -> pt*P*P*C).  ``last_keep`` holds the kept set
    [S, k] of the last forward; ``encoder_state_dict()`` is what ``ViViT.load_state_dict(strict=True)`` takes.  See the module
    docstring for what is and is not pre-trained."""

    def __init__(self, encoder: ViViT, *, decoder_dim: int = 384, decoder_depth: int = 4, decoder_heads: int = 6,
                 decoder_dim_head: int = 64, decoder_scale_dim: int = 4, mask_ratio: float = 0.9, mask_mode: str = "tube",
                 norm_pix_loss: bool = True):
        super().__init__()
        if not isinstance(encoder, ViViT):
            raise TypeError(f"encoder must be a ViViT, got {type(encoder).__name__}")
        if mask_mode not in ("tube", "frame"):
            raise ValueError(f"mask_mode must be 'tube' or 'frame', got {mask_mode!r}")
        if isinstance(mask_ratio, bool) or not isinstance(mask_ratio, (int, float)) or not 0.0 <= mask_ratio < 1.0:
            raise ValueError(f"mask_ratio must be a rate in [0, 1), got {mask_ratio!r}")
        if decoder_dim % 8:
            raise ValueError(f"decoder_dim = {decoder_dim} must be a multiple of 8")
        self.mask_ratio = float(mask_ratio)
        self.mask_mode = mask_mode
        self.norm_pix_loss = bool(norm_pix_loss)
        n = encoder.num_patches
        self.num_kept(n)                       # ValueError unless 1 <= k < n
        dim = encoder.to_patch_embedding[1].weight.shape[0]
        patch_dim = encoder.to_patch_embedding[1].weight.shape[1]
        tokens = encoder.num_frames // encoder.tubelet_size
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_dim))
        self.decoder_pos_embedding = nn.Parameter(torch.randn(1, tokens, n, decoder_dim) * 0.02)
        self.encoder = encoder
        self.decoder_embed = nn.Linear(dim, decoder_dim)
        self.decoder = Transformer(decoder_dim, decoder_depth, decoder_heads, decoder_dim_head,
                                   decoder_dim * decoder_scale_dim)
        self.decoder_pred = nn.Linear(decoder_dim, patch_dim)
        nn.init.normal_(self.mask_token, std=0.02)
        self.last_keep = None

    def num_kept(self, n: int) -> int:
        """k = n - floor(mask_ratio * n) (``ViViT.num_kept``'s rule); a masked autoencoder needs 1 <= k < n."""
        k = n - math.floor(self.mask_ratio * n)
        if not 1 <= k < n:
            raise ValueError(f"mask_ratio = {self.mask_ratio!r} keeps k = {k} of n = {n} patches; 1 <= k < n is needed "
                             "(something to encode and something to reconstruct)")
        return k

    def no_weight_decay(self):
        """Names ``optim.param_groups`` leaves undecayed besides the 1-D parameters: the encoder's set under the prefix it
        is registered with, the mask token and the decoder's positional table."""
        return {"encoder." + k for k in self.encoder.no_weight_decay()} | {"mask_token", "decoder_pos_embedding"}

    def encoder_state_dict(self):
        """The encoder's state dict under the ViViT's own keys: ``ViViT(...).load_state_dict(this, strict=True)``."""
        return self.encoder.state_dict()

    def _kept_rows(self, x, keep, S, t, n):
        """(keep [S, k], slot [S, n]): a caller's ``keep`` (checked on the host exactly as ``ViViT._kept_rows`` does: no
        device value is read), else a draw at a site of the dropout generator -- in training AND in eval."""
        from .. import ops
        if keep is not None:
            if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.int32 or keep.dim() != 2 or keep.shape[0] != S
                    or not 1 <= keep.shape[1] <= n):
                raise ValueError(f"keep must be an int32 tensor [{S}, k] with 1 <= k <= {n}, got "
                                 f"{getattr(keep, 'dtype', type(keep))} of shape {tuple(getattr(keep, 'shape', ()))}")
            if keep.device != x.device:
                raise ValueError(f"keep is on {keep.device}, the clip on {x.device}")
            if keep.shape[1] == n:
                raise ValueError(f"keep names all n = {n} positions: nothing is masked")
        if not x.is_cuda:
            raise RuntimeError("MaskedClipAutoencoder runs on the GPU (HIP device); there is no CPU path")
        if keep is not None:
            keep = keep.contiguous()
            return keep, ops.keep_slots(keep, n)
        k = self.num_kept(n)
        R, rows_per = (S // t, t) if self.mask_mode == "tube" else (S, 1)
        return ops.keep_draw(R, n, k, F._rng.tensor(x.device), F._rng.take(R * n), rows_per)

    def forward(self, x, keep=None):
        enc = self.encoder
        if x.dim() != 5:
            raise ValueError("MaskedClipAutoencoder expects a clip tensor [b, t, c, H, W]")
        b, t = x.shape[0], x.shape[1]
        if t != enc.num_frames:
            raise ValueError(f"clip has {t} frames but the encoder was built for {enc.num_frames}")
        pt, P, T = enc.tubelet_size, enc.patch_size, enc.compute_dtype
        t //= pt
        S = b * t
        n = (x.shape[3] // P) * (x.shape[4] // P)
        if n != enc.num_patches:
            raise ValueError(f"clip has {n} patch positions per frame but the encoder was built for {enc.num_patches}")
        F.lp_clear()
        keep, slot = self._kept_rows(x, keep, S, t, n)
        self.last_keep = keep
        k = keep.shape[1]
        pe = enc.to_patch_embedding[1]
        emb = F.patch_embed_keep(x, pe.weight, pe.bias, P, T, pt, keep, slot)
        tok = F.tokens_assemble_keep(emb, enc.space_token, enc.pos_embedding, keep, slot, S, t)
        tok = F.dropout(tok, enc.emb_dropout_p, self.training)
        z = enc.space_transformer(tok)                                   # every layer on every row, final norm included
        z = F.linear(z, self.decoder_embed.weight, self.decoder_embed.bias)                     # [S, k + 1, decoder_dim]
        full = F.tokens_restore(z, self.mask_token, self.decoder_pos_embedding, keep, slot, S, t, skip=1)
        y = self.decoder(full)
        pred = F.linear(y, self.decoder_pred.weight, self.decoder_pred.bias)                    # [S, n, pt*P*P*C]
        loss, _ = F.mae_loss(pred, x, slot, k, P, pt, self.norm_pix_loss)
        return loss, pred, slot
