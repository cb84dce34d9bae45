"""Float64 CPU statement of masked-autoencoder pre-training on the ViViT tokeniser (csrc/mae.hip, functional.tokens_restore
/ mae_loss, models.mae.MaskedClipAutoencoder), pinned to the imported reference modules by tests/golden/mae.npz
(tools/gen_golden_mae.py).  It builds on tests/patchdrop_ref.py (kept sets, tokens) and tests/tubelet_ref.py (the gather) and
is written the way a device would NOT do it: the targets are the whole materialised patch matrix, the restore is a gather
and a ``where``, the adjoints are explicit index loops, the step is autograd in the dtype of its inputs.

  keep [S, k] int32 ascending, slot [S, n] int32 its inverse (-1 = dropped); sequence s = bi t' + tau.
"""
from __future__ import annotations

from typing import Dict

import torch

from oracle import clip_path as O
from tests import patchdrop_ref as PR
from tests import tubelet_ref as TR

Tensor = torch.Tensor
EPS = 1e-6


def restore(y: Tensor, mask: Tensor, pos: Tensor, slot: Tensor, skip: int = 1) -> Tensor:
    """y [S, skip + k, d], mask [d], pos [T, n, d], slot [S, n] -> [S, n, d]."""
    S, n = slot.shape
    d = y.shape[-1]
    T = pos.shape[0]
    idx = slot.long().clamp(min=0) + skip
    rows = y.gather(1, idx[:, :, None].expand(S, n, d))
    kept = (slot >= 0)[:, :, None]
    return torch.where(kept, rows, mask.reshape(1, 1, d).expand(S, n, d)) + pos[torch.arange(S) % T]


def restore_adjoint(dout: Tensor, keep: Tensor, slot: Tensor, T: int, skip: int = 1):
    """-> (dy [S, skip + k, d], dmask [d], dpos [T, n, d]), by loops over the index tables."""
    S, n, d = dout.shape
    k = keep.shape[1]
    dy = torch.zeros(S, skip + k, d, dtype=dout.dtype)
    dmask = torch.zeros(d, dtype=dout.dtype)
    dpos = torch.zeros(T, n, d, dtype=dout.dtype)
    for s in range(S):
        for i in range(k):
            dy[s, skip + i] = dout[s, int(keep[s, i])]
        dmask = dmask + dout[s][slot[s] < 0].sum(0)
        dpos[s % T] = dpos[s % T] + dout[s]
    return dy, dmask, dpos


def targets(clip: Tensor, P: int, pt: int, norm_pix: bool, eps: float = EPS) -> Tensor:
    """[b, t, C, H, W] -> [S, n, D]: every row of the tubelet gather, per-patch normalised (mean and UNBIASED variance over
    the D values of a patch: ``torch.var``'s default, the MAE definition) under ``norm_pix``."""
    b, t = clip.shape[0], clip.shape[1]
    S = b * t // pt
    full = TR.gather(clip, P, pt)
    full = full.reshape(S, full.shape[0] // S, full.shape[1])
    if norm_pix:
        mean = full.mean(dim=-1, keepdim=True)
        var = full.var(dim=-1, keepdim=True)
        full = (full - mean) / (var + eps) ** 0.5
    return full


def loss(pred: Tensor, clip: Tensor, slot: Tensor, P: int, pt: int, norm_pix: bool):
    """-> (loss, per_patch [S, n]): the mean over the dropped patches of the mean over D of (pred - target)^2; per_patch is 0
    at kept positions."""
    tgt = targets(clip, P, pt, norm_pix)
    dropped = (slot < 0).to(pred.dtype)
    per = ((pred - tgt) ** 2).mean(dim=-1) * dropped
    return per.sum() / dropped.sum(), per


def loss_grad(pred: Tensor, clip: Tensor, slot: Tensor, P: int, pt: int, norm_pix: bool, g: float = 1.0) -> Tensor:
    """d loss / d pred times ``g``, in closed form: g 2 / (M D) (pred - target) at dropped positions, 0 at kept ones."""
    tgt = targets(clip, P, pt, norm_pix)
    dropped = (slot < 0).to(pred.dtype)
    M, D = float(dropped.sum()), pred.shape[-1]
    return g * 2.0 / (M * D) * (pred - tgt) * dropped[:, :, None]


def masked_forward(x: Tensor, P: Dict[str, Tensor], keep: Tensor, *, patch: int, depth: int, heads: int, dec_depth: int,
                   dec_heads: int, pt: int = 1, norm_pix: bool = True):
    """The whole pre-training forward on the state dict ``P`` of a ``MaskedClipAutoencoder`` -> (loss, per_patch, pred):
    tokens of ALL positions, selection of the rows [0] + 1 + keep, the space stack with its final norm, decoder_embed, restore,
    the decoder, decoder_pred, the masked loss."""
    enc = {name[len("encoder."):]: v for name, v in P.items() if name.startswith("encoder.")}
    tok = PR.tokens(x, enc, patch, pt)
    b, t, n1, d = tok.shape
    S, k = keep.shape
    assert S == b * t
    rows = torch.cat((torch.zeros(S, 1, dtype=torch.int64), 1 + keep.long()), dim=1)
    sel = tok.reshape(S, n1, d).gather(1, rows[:, :, None].expand(S, k + 1, d))
    z = O.prenorm_transformer(sel, enc, "space_transformer.", depth, heads)
    z = O.linear(z, P["decoder_embed.weight"], P["decoder_embed.bias"])
    slot = PR.slots_of(keep, n1 - 1)
    dd = z.shape[-1]
    full = restore(z, P["mask_token"].reshape(dd), P["decoder_pos_embedding"].reshape(t, n1 - 1, dd), slot, skip=1)
    y = O.prenorm_transformer(full, P, "decoder.", dec_depth, dec_heads)
    pred = O.linear(y, P["decoder_pred.weight"], P["decoder_pred.bias"])
    ls, per = loss(pred, x, slot, patch, pt, norm_pix)
    return ls, per, pred


def masked_step(x: Tensor, P: Dict[str, Tensor], keep: Tensor, **kw):
    """(loss, per_patch, {name: gradient}) in the dtype of ``P``; only the parameters that have a gradient are listed (the
    encoder's temporal stack, temporal token and head are not part of the forward)."""
    leaves = {name: v.detach().clone().requires_grad_(True) for name, v in P.items()}
    ls, per, _ = masked_forward(x, leaves, keep, **kw)
    grads = torch.autograd.grad(ls, list(leaves.values()), allow_unused=True)
    return ls.detach(), per.detach(), {name: g for name, g in zip(leaves, grads) if g is not None}
