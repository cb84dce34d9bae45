"""Drop-in mirror of the reference's ``src/models/vit.py`` on MI355X kernels.

Same class names, constructor signatures, ``forward`` signatures, submodule
layout and therefore the same ``state_dict`` keys as the reference
(``pos_embedding, space_token, temporal_token, to_patch_embedding.1.*,
{space,temporal}_transformer.layers.{i}.{0,1}.{norm,fn...}``, ``mlp_head.{0,1}.*``;
reference: src/models/vit.py:8-128), so reference checkpoints load unchanged.
``nn.Linear`` / ``nn.LayerNorm`` instances are parameter containers only: every
forward/backward runs through the HIP kernels of libdvt_hip.so (functional.py);
there is no torch arithmetic and no CPU path.

Build-side additions (keyword-only, defaults keep reference behaviour):
``compute_dtype`` -- activation / GEMM dtype (torch.bfloat16 default, torch.float32
for the fp32 parity mode); ``activation_checkpointing`` -- keep one activation per
transformer block and recompute the block in backward (BASELINE configs[4]);
``tubelet_size`` -- pt > 1 replaces the per-frame tokeniser by the ViViT paper's tubelet embedding (a pt x P x P patch
across pt consecutive frames, csrc/patchify.hip): the space stack runs on ``num_frames / pt`` temporal tokens.  The
state-dict keys stay the reference's; ``to_patch_embedding.1.weight`` is ``[dim, pt*P*P*C]`` and ``pos_embedding``
``[1, num_frames // pt, n + 1, dim]``.  ``ViViT.load_frame_checkpoint`` carries a per-frame checkpoint into such a model
(``inflate_patch_embedding``).
``patch_dropout`` / ``patch_dropout_mode`` -- in training, the space stack runs on a random subset of
k = n - floor(patch_dropout * n) patch tokens per sequence (csrc/patch_dropout.hip): ``"tube"`` keeps the same positions in
every temporal token of a clip (VideoMAE's tube masking), ``"frame"`` draws per temporal token (PatchDropout).  ``forward``
and ``loss`` also take a caller's ``keep [S, k]`` (int32, ascending rows), used as given in training and in eval.
``drop_path`` / ``drop_path_mode`` -- stochastic depth in training (csrc/drop_path.hip).  The rate rises linearly from 0 to
``drop_path`` over the 2 * depth layers in execution order (space stack first; timm's ``linspace`` rule); the attention
branch and the MLP branch of a layer draw independently at the layer's rate p.  ``"subset"``: a branch runs on exactly
k = S - floor(p S) of the S sequences of its stack, drawn on the device, and is added back scaled by S / k (DINOv2's
efficient stochastic depth) -- S = b * t' in the space stack and S = b in the temporal stack, so at b = 8 a rate below 1/8
drops nothing there; S <= 1024.  ``"bernoulli"``: timm's rule -- every sequence is dropped independently with probability
p, the branch runs on all of them, scale 1 / (1 - p).  ``ViViT.drop_keep`` (None, or one entry per residual branch in
execution order: 2 * depth of the space stack, then 2 * depth of the temporal stack; an entry is None -- the branch runs
fused on all sequences -- or an int32 device tensor [k] of ascending unique sequence indices) replaces the draws, in
training and in eval; it is checked on the host for type, shape and device only.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .. import functional as F

_BY_RATE = object()       # "no plan of this forward is known: judge stochastic depth by the rates"


class Patchify(nn.Module):
    """Position 0 of ``to_patch_embedding`` (the reference's einops ``Rearrange``,
    vit.py:90).  Parameter-free; the gather itself is fused into ``F.patch_embed``."""

    def __init__(self, patch_size: int, tubelet_size: int = 1):
        super().__init__()
        self.patch_size = patch_size
        self.tubelet_size = tubelet_size

    def forward(self, x):  # only reached when used stand-alone
        from .. import ops
        b, t = x.shape[0], x.shape[1]
        out = ops.tubelet_patchify(x, self.patch_size, self.tubelet_size, x.dtype)
        return out.view(b, t // self.tubelet_size, -1, out.shape[-1])


def inflate_patch_embedding(weight2d, tubelet_size: int, mode: str = "central"):
    """Per-frame patch-embedding weight [dim, P*P*C] -> tubelet weight [dim, pt*P*P*C] (block k = columns
    ``k*P*P*C : (k+1)*P*P*C``, the frame k of a tubelet).  ``"central"``: the weight in block ``pt // 2``, zeros elsewhere
    -- on a clip x the tubelet embedding then equals the per-frame embedding of ``x[:, pt//2::pt]``.  ``"average"``:
    ``weight / pt`` in every block -- the per-frame embedding of the mean frame of each tubelet.  Host-side, init-time."""
    if mode not in ("central", "average"):
        raise ValueError(f"inflate_patch_embedding: mode must be 'central' or 'average', got {mode!r}")
    if int(tubelet_size) != tubelet_size or tubelet_size < 1:
        raise ValueError(f"inflate_patch_embedding: tubelet_size must be an integer >= 1, got {tubelet_size!r}")
    if weight2d.dim() != 2:
        raise ValueError(f"inflate_patch_embedding: expected a weight [dim, P*P*C], got shape {tuple(weight2d.shape)}")
    pt = int(tubelet_size)
    d, pd = weight2d.shape
    w = weight2d.detach()
    if mode == "average":
        return (w / pt).repeat(1, pt)
    out = torch.zeros((d, pt * pd), dtype=w.dtype, device=w.device)
    out[:, (pt // 2) * pd:(pt // 2 + 1) * pd] = w
    return out


class GELU(nn.Module):
    """Exact-erf GELU (vit.py:22); fused into the GEMM epilogue inside FeedForward."""

    def forward(self, x):
        return F.gelu(x)


class PreNorm(nn.Module):
    """vit.py:8-14."""

    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward(self, x, **kwargs):
        if isinstance(self.fn, (Attention, FeedForward)) and not kwargs:
            return self.fn(x, _norm=self.norm)
        return self.fn(F.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps), **kwargs)


class FeedForward(nn.Module):
    """vit.py:17-28: Linear(dim, hidden) - GELU - Dropout - Linear(hidden, dim) - Dropout."""

    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(dim, hidden_dim),
            GELU(),
            nn.Dropout(dropout),
            nn.Linear(hidden_dim, dim),
            nn.Dropout(dropout),
        )
        self.dropout_p = dropout

    def forward(self, x, _norm=None, _residual=False, _cdt=None):
        # _cdt: GEMM operand type when x is an fp32 residual stream (the launch-bound temporal stack, see ViViT.forward)
        l1, l2 = self.net[0], self.net[3]
        if self.training and self.dropout_p > 0.0:         # unfused: Linear - GELU - Dropout - Linear - Dropout (:20-26)
            h = F.layernorm(x, _norm.weight, _norm.bias, _norm.eps) if _norm is not None else x
            h = F.dropout(F.gelu(F.linear(h, l1.weight, l1.bias)), self.dropout_p, True)
            y = F.dropout(F.linear(h, l2.weight, l2.bias), self.dropout_p, True)
            return F.add(x, y) if _residual else y
        return F.mlp_block(x, _norm.weight if _norm is not None else None,
                           _norm.bias if _norm is not None else None,
                           l1.weight, l1.bias, l2.weight, l2.bias, act="gelu",
                           prenorm=_norm is not None, residual=_residual,
                           eps=_norm.eps if _norm is not None else 1e-5, cdt=_cdt)


class Attention(nn.Module):
    """vit.py:30-58."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner_dim = dim_head * heads
        project_out = not (heads == 1 and dim_head == dim)
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(
            nn.Linear(inner_dim, dim),
            nn.Dropout(dropout),
        ) if project_out else nn.Identity()
        self.project_out = project_out
        self.dropout_p = dropout

    def forward(self, x, _norm=None, _residual=False, _cdt=None):
        w_out = self.to_out[0].weight if self.project_out else None
        b_out = self.to_out[0].bias if self.project_out else None
        if self.training and self.dropout_p > 0.0 and self.project_out:     # to_out = Linear + Dropout (:41-44)
            y = F.attn_block(x, _norm.weight if _norm is not None else None, _norm.bias if _norm is not None else None,
                             self.to_qkv.weight, w_out, b_out, self.heads, prenorm=_norm is not None, residual=False,
                             eps=_norm.eps if _norm is not None else 1e-5)
            y = F.dropout(y, self.dropout_p, True)
            return F.add(x, y) if _residual else y
        return F.attn_block(x, _norm.weight if _norm is not None else None,
                            _norm.bias if _norm is not None else None,
                            self.to_qkv.weight, w_out, b_out, self.heads,
                            prenorm=_norm is not None, residual=_residual,
                            eps=_norm.eps if _norm is not None else 1e-5, cdt=_cdt)


class Transformer(nn.Module):
    """vit.py:60-75: depth x [x = attn(LN x) + x; x = ff(LN x) + x], final LayerNorm."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0., drop_path=None):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.norm = nn.LayerNorm(dim)
        self.checkpoint = False          # build-side: recompute each block in backward (saves ~11 of 12 activations)
        rates = [0.0] * depth if drop_path is None else [float(p) for p in drop_path]
        if len(rates) != depth or not all(0.0 <= p < 1.0 for p in rates):
            raise ValueError(f"drop_path must be {depth} per-layer rates in [0, 1), got {drop_path!r}")
        self.drop_path_rates = rates     # build-side: stochastic depth of layer i's two branches (no parameter, no buffer)
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout)),
                PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout)),
            ]))

    def _drop_live(self, plan, rates) -> bool:
        """Does stochastic depth act on the branches ``rates`` / ``plan`` speak of?  Without a plan: while training at a
        non-zero rate.  With the plan of a forward (a caller's ``drop_keep``): where an entry names a subset."""
        if plan is _BY_RATE:
            return self.training and any(p > 0.0 for p in rates)
        return plan is not None and any(e is not None for e in plan)

    def stream_f32_ok(self, rows: int, cdt: torch.dtype) -> bool:
        """May this stack run on an fp32 residual stream with ``cdt`` GEMM operands for ``rows`` rows?  (The launch-bound
        zone: 16-bit kernels, no active dropout, and every residual GEMM of a block a launch-bound shape -- the fp32
        residual epilogue is the panel-streaming kernel's.)"""
        if cdt not in (torch.bfloat16, torch.float16) or len(self.layers) == 0:
            return False
        attn, ff = self.layers[0][0].fn, self.layers[0][1].fn
        if not attn.project_out or (self.training and (attn.dropout_p > 0.0 or ff.dropout_p > 0.0)):
            return False
        d, inner, hidden = attn.to_out[0].weight.shape[0], attn.to_out[0].weight.shape[1], ff.net[0].weight.shape[0]
        from .. import ops
        return ops.gemm_is_launch_bound(rows, d, inner, cdt) and ops.gemm_is_launch_bound(rows, d, hidden, cdt)

    def _block(self, attn, ff, cdt, da, df):
        """x -> one layer.  da / df: None (the fused residual route) or (keep, slot, alpha, gather_input) -- the attention /
        feed-forward branch on a subset of the sequences (F.drop_path_block; the blocks give their un-added form)."""
        def a_branch(t):
            return attn.fn(t, _norm=attn.norm, _residual=False, _cdt=cdt)

        def f_branch(t):
            return ff.fn(t, _norm=ff.norm, _residual=False, _cdt=cdt)

        def block(t):
            if da is None:
                t = attn.fn(t, _norm=attn.norm, _residual=True, _cdt=cdt)
            else:
                t = F.drop_path_block(t, a_branch, da[0], da[1], da[2], tuple(attn.parameters()), da[3])
            if df is None:
                return ff.fn(t, _norm=ff.norm, _residual=True, _cdt=cdt)
            return F.drop_path_block(t, f_branch, df[0], df[1], df[2], tuple(ff.parameters()), df[3])
        return block

    def forward_layers(self, x, cdt=None, drops=None):
        """All residual blocks, without the final norm.  cdt: GEMM operand type when x is an fp32 stream.  drops: None, or
        one entry per residual branch in execution order (2 per layer), as ``_block`` takes them -- made before the blocks
        run, so a checkpointed block recomputes on the subset it ran on."""
        for i, (attn, ff) in enumerate(self.layers):
            da, df = (None, None) if drops is None else (drops[2 * i], drops[2 * i + 1])
            if da is None and df is None:
                if self.checkpoint and self.training and torch.is_grad_enabled():
                    def block(t, attn=attn, ff=ff):
                        t = attn.fn(t, _norm=attn.norm, _residual=True, _cdt=cdt)
                        return ff.fn(t, _norm=ff.norm, _residual=True, _cdt=cdt)
                    x = F.checkpoint(block, x, tuple(attn.parameters()) + tuple(ff.parameters()))
                else:
                    x = attn.fn(x, _norm=attn.norm, _residual=True, _cdt=cdt)
                    x = ff.fn(x, _norm=ff.norm, _residual=True, _cdt=cdt)
                continue
            block = self._block(attn, ff, cdt, da, df)
            if self.checkpoint and self.training and torch.is_grad_enabled():
                x = F.checkpoint(block, x, tuple(attn.parameters()) + tuple(ff.parameters()))
            else:
                x = block(x)
        return x

    def cls_prunable(self, plan=_BY_RATE) -> bool:
        """True when the last layer may be evaluated for row 0 only (``forward_layers_cls``)."""
        if len(self.layers) == 0:
            return False
        attn = self.layers[-1][0].fn
        dropping = self.training and (attn.dropout_p > 0.0 or self.layers[-1][1].fn.dropout_p > 0.0)
        if self._drop_live(plan if plan is _BY_RATE or plan is None else plan[-2:], self.drop_path_rates[-1:]):
            dropping = True                                                  # the CLS route has no un-added form
        return attn.project_out and not dropping

    def forward_layers_cls(self, x, cdt=None, drops=None):
        """``forward_layers(x)[:, 0]`` for x [S, N, d] -> [S, d]: what the reference reads of the space
        transformer (vit.py:119-120) and, under pool == 'cls', of the temporal one (:126).  In the last
        layer only the keys and values are computed for all rows; query, attention, output projection and
        the whole feed-forward run on row 0 of every sequence (F.attn_block_cls)."""
        *head, (attn, ff) = self.layers
        if drops is not None and (drops[-1] is not None or drops[-2] is not None):
            raise ValueError("drop_path: the CLS route of the last layer has no un-added form")
        for i, (a, f) in enumerate(head):
            da, df = (None, None) if drops is None else (drops[2 * i], drops[2 * i + 1])
            if da is not None or df is not None:
                block = self._block(a, f, cdt, da, df)
                x = (F.checkpoint(block, x, tuple(a.parameters()) + tuple(f.parameters()))
                     if self.checkpoint and self.training and torch.is_grad_enabled() else block(x))
            elif self.checkpoint and self.training and torch.is_grad_enabled():
                def block(t, a=a, f=f):
                    t = a.fn(t, _norm=a.norm, _residual=True, _cdt=cdt)
                    return f.fn(t, _norm=f.norm, _residual=True, _cdt=cdt)
                x = F.checkpoint(block, x, tuple(a.parameters()) + tuple(f.parameters()))
            else:
                x = a.fn(x, _norm=a.norm, _residual=True, _cdt=cdt)
                x = f.fn(x, _norm=f.norm, _residual=True, _cdt=cdt)

        def last(t):
            an, af = attn.norm, attn.fn
            c = F.attn_block_cls(t, an.weight, an.bias, af.to_qkv.weight, af.to_out[0].weight, af.to_out[0].bias,
                                 af.heads, eps=an.eps, cdt=cdt)
            return ff.fn(c, _norm=ff.norm, _residual=True, _cdt=cdt)

        if self.checkpoint and self.training and torch.is_grad_enabled():
            return F.checkpoint(last, x, tuple(attn.parameters()) + tuple(ff.parameters()))
        return last(x)

    def forward(self, x, cdt=None, drops=None):
        x = self.forward_layers(x, cdt, drops)
        return F.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps)


class ViViT(nn.Module):
    """vit.py:79-128.  ``forward(x[b, t, c, H, W]) -> [b, num_classes]`` (fp32 logits)."""

    def __init__(self, image_size, patch_size, num_classes, num_frames, dim=192, depth=4, heads=3,
                 pool='cls', in_channels=3, dim_head=64, dropout=0., emb_dropout=0., scale_dim=4, *,
                 compute_dtype: torch.dtype = torch.bfloat16, activation_checkpointing: bool = False,
                 patch_dropout: float = 0.0, patch_dropout_mode: str = "tube", drop_path: float = 0.0,
                 drop_path_mode: str = "subset", tubelet_size: int = 1):
        super().__init__()
        assert pool in {'cls', 'mean'}, 'pool type must be either cls (cls token) or mean (mean pooling)'
        assert image_size % patch_size == 0, 'Image dimensions must be divisible by the patch size.'
        if isinstance(tubelet_size, bool) or not isinstance(tubelet_size, int) or tubelet_size < 1:
            raise ValueError(f"tubelet_size must be an integer >= 1, got {tubelet_size!r}")
        if num_frames % tubelet_size != 0:
            raise ValueError(f"num_frames = {num_frames} is not a multiple of tubelet_size = {tubelet_size}")
        num_patches = (image_size // patch_size) ** 2
        if patch_dropout_mode not in ("tube", "frame"):
            raise ValueError(f"patch_dropout_mode must be 'tube' or 'frame', got {patch_dropout_mode!r}")
        self.patch_dropout = float(patch_dropout)
        self.patch_dropout_mode = patch_dropout_mode
        self.num_kept(num_patches)             # ValueError unless 0 <= patch_dropout < 1 and k >= 1
        if isinstance(drop_path, bool) or not isinstance(drop_path, (int, float)) or not 0.0 <= drop_path < 1.0:
            raise ValueError(f"drop_path must be a rate in [0, 1), got {drop_path!r}")
        if drop_path_mode not in ("subset", "bernoulli"):
            raise ValueError(f"drop_path_mode must be 'subset' or 'bernoulli', got {drop_path_mode!r}")
        self.drop_path = float(drop_path)
        self.drop_path_mode = drop_path_mode
        self.drop_keep = None                  # a caller's subsets, one entry per residual branch (see the module docstring)
        self.last_drop_plan = None             # what the last forward ran on: per branch None or (keep, slot, alpha, gather)
        rates = self.drop_path_rates(depth, self.drop_path)
        patch_dim = tubelet_size * in_channels * patch_size ** 2
        self.to_patch_embedding = nn.Sequential(
            Patchify(patch_size, tubelet_size),
            nn.Linear(patch_dim, dim),
        )
        self.pos_embedding = nn.Parameter(torch.randn(1, num_frames // tubelet_size, num_patches + 1, dim))
        self.space_token = nn.Parameter(torch.randn(1, 1, dim))
        self.space_transformer = Transformer(dim, depth, heads, dim_head, dim * scale_dim, dropout, rates[:depth])
        self.temporal_token = nn.Parameter(torch.randn(1, 1, dim))
        self.temporal_transformer = Transformer(dim, depth, heads, dim_head, dim * scale_dim, dropout, rates[depth:])
        self.dropout = nn.Dropout(emb_dropout)
        self.pool = pool
        self.mlp_head = nn.Sequential(
            nn.LayerNorm(dim),
            nn.Linear(dim, num_classes),
        )
        self.patch_size = patch_size
        self.num_patches = num_patches
        self.num_frames = num_frames          # pixel frames of a clip; the stacks see num_frames // tubelet_size of them
        self.tubelet_size = tubelet_size
        self.emb_dropout_p = emb_dropout
        self.compute_dtype = compute_dtype
        self.zone_f32 = True          # fp32 residual stream in the temporal stack / heads under 16-bit kernels (see forward)
        self.space_transformer.checkpoint = activation_checkpointing
        self.temporal_transformer.checkpoint = activation_checkpointing

    # ---- the fine-tuning grouping (optim.param_groups): what is not decayed, and the layer of every parameter
    def no_weight_decay(self):
        """Parameters with more than one dimension that weight decay leaves alone all the same (timm's convention)."""
        return {"pos_embedding", "space_token", "temporal_token"}

    @property
    def num_lr_layers(self) -> int:
        """The layer id of the head under layer-wise learning-rate decay: both stacks' depths + 1."""
        return len(self.space_transformer.layers) + len(self.temporal_transformer.layers) + 1

    def layer_id(self, name: str) -> int:
        """Layer of the parameter ``name`` in execution order, 0 (patch embedding) .. ``num_lr_layers`` (head): space layer i
        is i + 1, the space stack's final norm shares the last space layer's id, the temporal token opens the temporal
        stack, temporal layer j is Ds + 1 + j, and the temporal stack's final norm goes with the head."""
        Ds, Dt = len(self.space_transformer.layers), len(self.temporal_transformer.layers)
        if name in ("pos_embedding", "space_token") or name.startswith("to_patch_embedding."):
            return 0
        if name == "temporal_token":
            return Ds + 1
        if name.startswith("space_transformer.norm."):
            return Ds
        if name.startswith("temporal_transformer.norm.") or name.startswith("mlp_head."):
            return Ds + Dt + 1
        for prefix, base, depth in (("space_transformer.layers.", 1, Ds), ("temporal_transformer.layers.", Ds + 1, Dt)):
            if name.startswith(prefix):
                i = name[len(prefix):].split(".", 1)[0]
                if i.isdigit() and int(i) < depth:
                    return base + int(i)
        raise KeyError(f"ViViT.layer_id: {name!r} is not a parameter of this model")

    def num_kept(self, n: int) -> int:
        """k = n - floor(patch_dropout * n): the patch tokens a sequence of n positions keeps in training."""
        p = self.patch_dropout
        if not 0.0 <= p < 1.0:
            raise ValueError(f"patch_dropout must be in [0, 1), got {p!r}")
        k = n - math.floor(p * n)
        if k < 1:
            raise ValueError(f"patch_dropout = {p!r} keeps no patch of {n}")
        return k

    @staticmethod
    def drop_path_rates(depth: int, drop_path: float):
        """The rate of each of the 2 * depth layers in execution order (space stack first): linear from 0 to ``drop_path``
        (timm: ``torch.linspace(0, drop_path_rate, number of layers)``)."""
        n = 2 * depth
        return [drop_path * i / (n - 1) if n > 1 else drop_path for i in range(n)]

    @staticmethod
    def drop_path_kept(S: int, p: float) -> int:
        """k = S - floor(p S): the sequences of a stack of S a branch at rate p runs on in ``"subset"`` mode."""
        if not 0.0 <= p < 1.0:
            raise ValueError(f"drop_path: rate {p!r} outside [0, 1)")
        return S - math.floor(p * S)

    def forward(self, x, keep=None):
        pooled, pending = self._trunk(x, keep)
        if pending is not None:                                                     # the temporal stack's final norm (:43)
            pooled = F.layernorm(pooled, pending.weight, pending.bias, pending.eps)
        hn, hl = self.mlp_head[0], self.mlp_head[1]
        h = F.layernorm(pooled, hn.weight, hn.bias, hn.eps)
        return F.linear(h, hl.weight, hl.bias, out_f32=True)                        # :128

    def loss(self, x, target, keep=None):
        """nn.BCEWithLogitsLoss()(self(x), target) (the training step of the reference's Lightning wrapper), with the head
        -- final norm on the pooled row, mlp_head, the loss -- as one launch where the shape allows (8 rows at the metric
        shape: the separate kernels are pure launch cost).  -> (loss, logits)."""
        pooled, pending = self._trunk(x, keep)
        hn, hl = self.mlp_head[0], self.mlp_head[1]
        if pooled.is_cuda and F.head_bce_supported(pooled, hl.weight):
            mixed = pooled.dtype == torch.float32 and self.compute_dtype in (torch.bfloat16, torch.float16)
            return F.head_bce(pooled, pending, hn, hl, target, lp_dtype=self.compute_dtype if mixed else None)
        if pending is not None:
            pooled = F.layernorm(pooled, pending.weight, pending.bias, pending.eps)
        logits = F.linear(F.layernorm(pooled, hn.weight, hn.bias, hn.eps), hl.weight, hl.bias, out_f32=True)
        return F.bce_with_logits(logits, target), logits

    def load_frame_checkpoint(self, state_dict, mode: str = "central"):
        """Load the state dict of a per-frame ``ViViT`` (``tubelet_size=1``) of the same geometry and ``num_frames`` into
        this tubelet model: ``to_patch_embedding.1.weight`` is inflated (``inflate_patch_embedding``), ``pos_embedding``
        is reduced over time -- rows ``pt//2::pt`` for ``"central"``, the mean over each group of pt rows for
        ``"average"`` -- and every other tensor is copied strictly.  ValueError, naming the key, on any key or shape
        mismatch; nothing is written before every tensor has been checked."""
        if mode not in ("central", "average"):
            raise ValueError(f"load_frame_checkpoint: mode must be 'central' or 'average', got {mode!r}")
        pt = self.tubelet_size
        own = self.state_dict()
        for k in own:
            if k not in state_dict:
                raise ValueError(f"load_frame_checkpoint: key {k!r} is missing from the checkpoint")
        for k in state_dict:
            if k not in own:
                raise ValueError(f"load_frame_checkpoint: unexpected key {k!r} in the checkpoint")
        new = {}
        for k, dst in own.items():
            src = state_dict[k].detach()
            if k == "to_patch_embedding.1.weight":
                if src.dim() != 2 or (src.shape[0], src.shape[1] * pt) != tuple(dst.shape):
                    raise ValueError(f"load_frame_checkpoint: {k!r} has shape {tuple(src.shape)}; a per-frame weight "
                                     f"[{dst.shape[0]}, {dst.shape[1] // pt}] is expected")
                src = inflate_patch_embedding(src, pt, mode)
            elif k == "pos_embedding":
                want = (1, self.num_frames) + tuple(dst.shape[2:])
                if tuple(src.shape) != want:
                    raise ValueError(f"load_frame_checkpoint: {k!r} has shape {tuple(src.shape)}; the per-frame table "
                                     f"{want} is expected")
                if mode == "central":
                    src = src[:, pt // 2::pt]
                else:
                    src = src.reshape(1, self.num_frames // pt, pt, *src.shape[2:]).mean(2)
            elif tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"load_frame_checkpoint: {k!r} has shape {tuple(src.shape)}, the model's is "
                                 f"{tuple(dst.shape)}")
            new[k] = src
        with torch.no_grad():
            for k, dst in own.items():
                dst.copy_(new[k])

    def _kept_rows(self, x, keep, S, t, n):
        """-> (keep [S, k], slot [S, n]) or (None, None): a caller's ``keep`` as given (checked on the host: no device value
        is read), else -- in training with patch_dropout > 0 -- a draw at a site of the dropout generator."""
        if keep is not None:
            if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.int32 or keep.dim() != 2 or keep.shape[0] != S
                    or not 1 <= keep.shape[1] <= n):
                raise ValueError(f"keep must be an int32 tensor [{S}, k] with 1 <= k <= {n}, got "
                                 f"{getattr(keep, 'dtype', type(keep))} of shape {tuple(getattr(keep, 'shape', ()))}")
            if keep.device != x.device:
                raise ValueError(f"keep is on {keep.device}, the clip on {x.device}")
            from .. import ops
            keep = keep.contiguous()
            return keep, ops.keep_slots(keep, n)
        if not (self.training and self.patch_dropout > 0.0):
            return None, None
        from .. import ops
        k = self.num_kept(n)
        R, rows_per = (S // t, t) if self.patch_dropout_mode == "tube" else (S, 1)
        return ops.keep_draw(R, n, k, F._rng.tensor(x.device), F._rng.take(R * n), rows_per)

    def _drop_plan(self, x, S_space: int, S_time: int):
        """-> (space entries, temporal entries, by_caller): per residual branch None (fused, all sequences) or
        (keep, slot, alpha, gather_input), or (None, None, False) when stochastic depth does not act.  Every subset is made
        here, before any block runs.  A caller's ``drop_keep`` is checked on the host only: no device value is read."""
        from .. import ops
        st, tt = self.space_transformer, self.temporal_transformer
        nb = 2 * len(st.layers)
        stacks = ((st, S_space), (tt, S_time))
        dk = self.drop_keep
        if dk is not None:
            if not isinstance(dk, (list, tuple)) or len(dk) != 2 * nb:
                raise ValueError(f"drop_keep must be a sequence of {2 * nb} entries (one per residual branch: {nb} of the "
                                 f"space stack, then {nb} of the temporal stack), got "
                                 f"{len(dk) if isinstance(dk, (list, tuple)) else type(dk).__name__}")
            plans = []
            for si, (stack, S) in enumerate(stacks):
                plan = []
                for j in range(nb):
                    e = dk[si * nb + j]
                    if e is None:
                        plan.append(None)
                        continue
                    if (not isinstance(e, torch.Tensor) or e.dtype != torch.int32 or e.dim() != 1
                            or not 1 <= e.numel() <= S):
                        raise ValueError(f"drop_keep[{si * nb + j}] must be None or an int32 tensor [k] with 1 <= k <= {S}, "
                                         f"got {getattr(e, 'dtype', type(e))} of shape {tuple(getattr(e, 'shape', ()))}")
                    if e.device != x.device:
                        raise ValueError(f"drop_keep[{si * nb + j}] is on {e.device}, the clip on {x.device}")
                    if S > ops.DROP_PATH_MAX_SEQS:
                        raise ValueError(f"drop_keep: a subset of S = {S} sequences; the limit is {ops.DROP_PATH_MAX_SEQS}")
                    e = e.contiguous()
                    k = e.numel()
                    p = stack.drop_path_rates[j // 2]
                    alpha = S / k if self.drop_path_mode == "subset" else 1.0 / (1.0 - p)
                    plan.append((e, ops.keep_slots(e.view(1, k), S).view(S), alpha, True))
                plans.append(plan)
            return plans[0], plans[1], True
        if not (self.training and self.drop_path > 0.0):
            return None, None, False
        state = F._rng.tensor(x.device)
        plans = []
        for stack, S in stacks:
            plan = []
            for j in range(nb):
                p = stack.drop_path_rates[j // 2]
                if self.drop_path_mode == "bernoulli":
                    if p > 0.0:
                        m = ops.drop_path_draw(S, p, state, F._rng.take(S))
                        plan.append((m, m, 1.0 / (1.0 - p), False))
                    else:
                        plan.append(None)
                    continue
                if p > 0.0 and S > ops.DROP_PATH_MAX_SEQS:
                    raise ValueError(f"drop_path_mode='subset' draws from at most {ops.DROP_PATH_MAX_SEQS} sequences, this "
                                     f"stack has S = {S}; use drop_path_mode='bernoulli' or a smaller batch")
                k = self.drop_path_kept(S, p)
                if k == S:
                    plan.append(None)
                else:
                    kp, sl = ops.keep_draw(1, S, k, state, F._rng.take(S))
                    plan.append((kp.view(k), sl.view(S), S / k, True))
            plans.append(plan)
        return plans[0], plans[1], False

    def _trunk(self, x, keep=None):
        """-> (pooled [b, dim], the LayerNorm still to be applied to it or None)."""
        if x.dim() != 5:
            raise ValueError("ViViT expects a clip tensor [b, t, c, H, W]")
        b, t = x.shape[0], x.shape[1]
        if t != self.num_frames:
            raise ValueError(f"clip has {t} frames but pos_embedding was built for {self.num_frames} "
                             "(vit.py:94,115 broadcast)")
        t //= self.tubelet_size                 # temporal tokens: everything below sees a clip of t tubelets
        T = self.compute_dtype
        F.lp_clear()            # 16-bit gradient copies a previous step's backward left untaken (functional._lp_hand)
        sd, td, planned = self._drop_plan(x, b * t, b)          # stochastic depth: every subset of this step, or None
        self.last_drop_plan = None if sd is None else sd + td
        sp, tp = ((sd, td) if planned else (_BY_RATE, _BY_RATE))
        n = (x.shape[3] // self.patch_size) * (x.shape[4] // self.patch_size)
        pe = self.to_patch_embedding[1]
        keep, slot = self._kept_rows(x, keep, b * t, t, n)
        if keep is None:
            emb = F.patch_embed(x, pe.weight, pe.bias, self.patch_size, T, tubelet=self.tubelet_size)   # vit.py:110
            tok = F.tokens_assemble(emb, self.space_token, self.pos_embedding, b * t, t, n)   # :113-115
        else:                                               # the same two lines on the kept patch tokens
            emb = F.patch_embed_keep(x, pe.weight, pe.bias, self.patch_size, T, self.tubelet_size, keep, slot)
            tok = F.tokens_assemble_keep(emb, self.space_token, self.pos_embedding, keep, slot, b * t, t)
        tok = F.dropout(tok, self.emb_dropout_p, self.training)                            # :116
        st, tt = self.space_transformer, self.temporal_transformer
        sn = st.norm
        if st.cls_prunable(sp):                                                     # only x[:, 0] is read (:120)
            s = st.forward_layers_cls(tok, drops=sd).view(b * t, 1, -1)
        else:
            s = st.forward_layers(tok, drops=sd)                                    # :118-119
        # The temporal stack and the heads are the launch-bound zone of the step (b (t + 1) rows: 264 at the metric shape):
        # single rows carry whole gradients there and nothing averages the rounding of 16-bit storage, while fp32 storage
        # of so few rows costs no bandwidth -- its residual stream and row gradients are kept in fp32 (GEMM operands stay T).
        zone32 = self.zone_f32 and tt.stream_f32_ok(b * (t + 1), T)
        cdt = T if zone32 else None
        seq = F.cls_norm_concat(s, sn.weight, sn.bias, self.temporal_token, b, t, sn.eps,
                                out_dtype=torch.float32 if zone32 else None)       # :119-123
        if self.pool == 'cls' and tt.cls_prunable(tp):                              # only x[:, 0] is read (:126)
            return tt.forward_layers_cls(seq, cdt, td), tt.norm
        z = tt(seq, cdt, td)                                                        # :125
        return (F.mean_rows(z) if self.pool == 'mean' else F.select_first_row(z)), None  # :126
