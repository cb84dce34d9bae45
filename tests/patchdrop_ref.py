"""CPU reference of patch dropout on the ViViT: training on a kept subset of the patch tokens of every sequence (the same
positions in every frame of a clip: tube masking, as in VideoMAE; drawn per frame: PatchDropout).  A sequence
s = bi t' + tau keeps k of its n patch positions, ``keep[s]`` (strictly ascending); ``slot[s]`` is the inverse map, -1 for
a dropped position.  The library has no device implementation yet; this is the float64 statement one is to be held to,
itself pinned to the imported reference model by tests/golden/patch_dropout.npz (tools/gen_golden_patch_dropout.py).
It is written the way a device would NOT do it -- everything is computed for all n positions and dropped afterwards:

  * ``keep_select`` -- the rank rule as a stable argsort of the keys: the first k of the order (key, position);
  * ``gather_keep`` -- the full gather ``tubelet_ref.gather`` followed by row selection;
  * ``masked_forward`` -- the oracle's ``vivit_tokens`` (patch embedding, CLS, positional add on ALL n positions), then
    selection of the rows ``[0] + 1 + keep``, then the oracle's transformer, pooling and head, in float64 with autograd.
"""
from __future__ import annotations

from typing import Dict

import torch

from oracle import clip_path as O
from tests import tubelet_ref as TR

Tensor = torch.Tensor


def keep_select(keys: Tensor, k: int, rows_per: int = 1):
    """keys [R, n] (integers) -> (keep [R*rows_per, k] ascending int32, slot [R*rows_per, n] int32, -1 = dropped)."""
    R, n = keys.shape
    order = torch.argsort(keys.to(torch.int64), dim=1, stable=True)     # ties: the lower position first
    keep = torch.sort(order[:, :k], dim=1).values
    slot = torch.full((R, n), -1, dtype=torch.int64)
    slot.scatter_(1, keep, torch.arange(k).expand(R, k))
    return (keep.repeat_interleave(rows_per, dim=0).to(torch.int32).contiguous(),
            slot.repeat_interleave(rows_per, dim=0).to(torch.int32).contiguous())


def slots_of(keep: Tensor, n: int) -> Tensor:
    S, k = keep.shape
    slot = torch.full((S, n), -1, dtype=torch.int64)
    slot.scatter_(1, keep.long(), torch.arange(k).expand(S, k))
    return slot.to(torch.int32)


def gather_keep(x: Tensor, P: int, pt: int, keep: Tensor) -> Tensor:
    """[b, t, C, H, W], keep [S, k] -> [S k, pt P P C]: the full gather, then the kept rows."""
    full = TR.gather(x, P, pt)
    S, k = keep.shape
    n = full.shape[0] // S
    return full.reshape(S, n, -1).gather(1, keep.long()[:, :, None].expand(S, k, full.shape[1])).reshape(S * k, -1)


def scatter_keep(d: Tensor, shape, P: int, pt: int, keep: Tensor) -> Tensor:
    """The adjoint of ``gather_keep`` by autograd."""
    x = torch.zeros(tuple(shape), dtype=d.dtype, requires_grad=True)
    (gather_keep(x, P, pt, keep) * d).sum().backward()
    return x.grad


def tokens(x: Tensor, P: Dict[str, Tensor], patch: int, pt: int = 1) -> Tensor:
    """[b, t', n + 1, d]: the oracle's ``vivit_tokens``; for pt > 1 the same lines on the tubelet gather."""
    if pt == 1:
        return O.vivit_tokens(x, P, patch)
    b, t = x.shape[0], x.shape[1] // pt
    e = O.linear(TR.gather(x, patch, pt).reshape(b, t, -1, pt * patch * patch * x.shape[2]),
                 P["to_patch_embedding.1.weight"], P["to_patch_embedding.1.bias"])
    n, d = e.shape[2], e.shape[3]
    cls = P["space_token"].reshape(1, 1, 1, d).expand(b, t, 1, d)
    return torch.cat((cls, e), dim=2) + P["pos_embedding"][:, :, : n + 1]


def masked_forward(x: Tensor, P: Dict[str, Tensor], keep: Tensor, *, patch: int, depth: int, heads: int, pt: int = 1,
                   pool: str = "cls") -> Tensor:
    """``oracle.clip_path.vivit_forward`` with the space stack run on the rows [0] + 1 + keep[s] of sequence s."""
    tok = tokens(x, P, patch, pt)
    b, t, n1, d = tok.shape
    S, k = keep.shape
    assert S == b * t
    rows = torch.cat((torch.zeros(S, 1, dtype=torch.int64), 1 + keep.long()), dim=1)          # [S, k + 1]
    sel = tok.reshape(S, n1, d).gather(1, rows[:, :, None].expand(S, k + 1, d))
    s = O.prenorm_transformer(sel, P, "space_transformer.", depth, heads)
    frame_cls = s[:, 0].reshape(b, t, d)
    tcls = P["temporal_token"].reshape(1, 1, d).expand(b, 1, d)
    z = O.prenorm_transformer(torch.cat((tcls, frame_cls), dim=1), P, "temporal_transformer.", depth, heads)
    pooled = z.mean(dim=1) if pool == "mean" else z[:, 0]
    h = O.layernorm(pooled, P["mlp_head.0.weight"], P["mlp_head.0.bias"])
    return O.linear(h, P["mlp_head.1.weight"], P["mlp_head.1.bias"])


def masked_step(x: Tensor, target: Tensor, P: Dict[str, Tensor], keep: Tensor, **kw):
    """(logits, loss, {name: gradient}) of BCE-with-logits on ``masked_forward``, in the dtype of ``P`` (float64)."""
    leaves = {name: v.detach().clone().requires_grad_(True) for name, v in P.items()}
    logits = masked_forward(x, leaves, keep, **kw)
    loss = O.bce_with_logits(logits, target)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return logits.detach(), loss.detach(), {name: (g if g is not None else torch.zeros_like(leaves[name]))
                                            for name, g in zip(leaves, grads)}
