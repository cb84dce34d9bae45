"""JointViViT: joint space-time attention over all tubelet tokens of a clip (ViViT "Model 1"; the plain-ViT encoder of
VideoMAE), on the kernels of libdvt_hip.so.

The reference ships the factorised encoder only (src/models/vit.py:79-128); this model assembles the same parts -- the
``Rearrange`` + ``Linear`` patch embedding, a CLS token, a learned positional table, one ``Transformer`` (vit.py:60-75), the
``LayerNorm`` + ``Linear`` head -- into the unfactorised form: every one of the ``(num_frames // tubelet_size) * n`` patch
tokens of a clip, plus the CLS token, attends to every other in ONE stack.  At the metric clip with ``tubelet_size=2`` that is
3137 tokens per sequence; the dense layers run the streamed attention kernels (functional.ATTN_LONG, csrc/attention.hip
attn_long_*), the last layer's single CLS query under ``pool='cls'`` the Q1 kernels (``Transformer.forward_layers_cls``).

state_dict keys: ``pos_embedding`` [1, 1, t' n + 1, dim], ``cls_token`` [1, 1, dim], ``to_patch_embedding.1.*``,
``transformer.layers.{i}.{0,1}.*``, ``transformer.norm.*``, ``mlp_head.{0,1}.*``.

Not on this model: patch dropout and ``keep=``, stochastic depth, the masked-autoencoder decoder over
joint tokens, ``AttentionRollout``; ``compute_dtype=torch.float32`` runs, on the generic attention kernels.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as F
from .vit import Patchify, Transformer


class JointViViT(nn.Module):
    """``forward(x[b, t, c, H, W]) -> [b, num_classes]`` (fp32 logits)."""

    def __init__(self, image_size, patch_size, num_classes, num_frames, dim=192, depth=4, heads=3,
                 pool='cls', in_channels=3, dim_head=64, dropout=0., emb_dropout=0., scale_dim=4, *,
                 compute_dtype: torch.dtype = torch.bfloat16, activation_checkpointing: bool = False,
                 tubelet_size: int = 1):
        super().__init__()
        assert pool in {'cls', 'mean'}, 'pool type must be either cls (cls token) or mean (mean pooling)'
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        if isinstance(tubelet_size, bool) or not isinstance(tubelet_size, int) or tubelet_size < 1:
            raise ValueError(f"tubelet_size must be an integer >= 1, got {tubelet_size!r}")
        if num_frames % tubelet_size != 0:
            raise ValueError(f"num_frames = {num_frames} is not a multiple of tubelet_size = {tubelet_size}")
        num_patches = (image_size // patch_size) ** 2
        patch_dim = tubelet_size * in_channels * patch_size ** 2
        self.to_patch_embedding = nn.Sequential(
            Patchify(patch_size, tubelet_size),
            nn.Linear(patch_dim, dim),
        )
        self.num_tokens = (num_frames // tubelet_size) * num_patches        # patch tokens of a clip (without the CLS row)
        self.pos_embedding = nn.Parameter(torch.randn(1, 1, self.num_tokens + 1, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = Transformer(dim, depth, heads, dim_head, dim * scale_dim, dropout)
        self.pool = pool
        self.mlp_head = nn.Sequential(
            nn.LayerNorm(dim),
            nn.Linear(dim, num_classes),
        )
        self.image_size = image_size
        self.patch_size = patch_size
        self.num_patches = num_patches
        self.num_frames = num_frames
        self.tubelet_size = tubelet_size
        self.emb_dropout_p = emb_dropout
        self.compute_dtype = compute_dtype
        self.transformer.checkpoint = activation_checkpointing

    # ---- the fine-tuning grouping (optim.param_groups): what is not decayed, and the layer of every parameter
    def no_weight_decay(self):
        return {"pos_embedding", "cls_token"}

    @property
    def num_lr_layers(self) -> int:
        """The layer id of the head under layer-wise learning-rate decay: the stack's depth + 1."""
        return len(self.transformer.layers) + 1

    def layer_id(self, name: str) -> int:
        """Layer of the parameter ``name``: 0 (patch embedding, tokens), i + 1 for layer i of the stack, ``num_lr_layers``
        for the stack's final norm and the head."""
        D = len(self.transformer.layers)
        if name in ("pos_embedding", "cls_token") or name.startswith("to_patch_embedding."):
            return 0
        if name.startswith("transformer.norm.") or name.startswith("mlp_head."):
            return D + 1
        prefix = "transformer.layers."
        if name.startswith(prefix):
            i = name[len(prefix):].split(".", 1)[0]
            if i.isdigit() and int(i) < D:
                return 1 + int(i)
        raise KeyError(f"JointViViT.layer_id: {name!r} is not a parameter of this model")

    def _trunk(self, x):
        """-> (pooled [b, dim], the LayerNorm still to be applied to it or None)."""
        if x.dim() != 5:
            raise ValueError("JointViViT expects a clip tensor [b, t, c, H, W]")
        b, t = x.shape[0], x.shape[1]
        if t != self.num_frames:
            raise ValueError(f"clip has {t} frames but pos_embedding was built for {self.num_frames}")
        if x.shape[3] != self.image_size or x.shape[4] != self.image_size:
            raise ValueError(f"clip frames are {x.shape[3]} x {x.shape[4]} but pos_embedding was built for "
                             f"{self.image_size} x {self.image_size}")
        T = self.compute_dtype
        F.lp_clear()
        pe = self.to_patch_embedding[1]
        emb = F.patch_embed(x, pe.weight, pe.bias, self.patch_size, T, tubelet=self.tubelet_size)   # [b * t' * n, dim]
        tok = F.tokens_assemble(emb, self.cls_token, self.pos_embedding, b, 1, self.num_tokens)      # [b, t' n + 1, dim]
        tok = F.dropout(tok, self.emb_dropout_p, self.training)
        tr = self.transformer
        if self.pool == 'cls' and tr.cls_prunable():            # only row 0 of the stack's output is read
            return tr.forward_layers_cls(tok), tr.norm
        z = tr(tok)
        return (F.mean_rows(z) if self.pool == 'mean' else F.select_first_row(z)), None

    def forward(self, x):
        pooled, pending = self._trunk(x)
        if pending is not None:
            pooled = F.layernorm(pooled, pending.weight, pending.bias, pending.eps)
        hn, hl = self.mlp_head[0], self.mlp_head[1]
        return F.linear(F.layernorm(pooled, hn.weight, hn.bias, hn.eps), hl.weight, hl.bias, out_f32=True)

    def loss(self, x, target):
        """nn.BCEWithLogitsLoss()(self(x), target), with final norm, head and loss as one launch where the shape allows
        (as ``ViViT.loss``).  -> (loss, logits)."""
        pooled, pending = self._trunk(x)
        hn, hl = self.mlp_head[0], self.mlp_head[1]
        if pooled.is_cuda and F.head_bce_supported(pooled, hl.weight):
            return F.head_bce(pooled, pending, hn, hl, target)
        if pending is not None:
            pooled = F.layernorm(pooled, pending.weight, pending.bias, pending.eps)
        logits = F.linear(F.layernorm(pooled, hn.weight, hn.bias, hn.eps), hl.weight, hl.bias, out_f32=True)
        return F.bce_with_logits(logits, target), logits
