"""``SSLEvaluator``: the MLP probe that the reference's ``SSLOnlineEval`` callback (src/callbacks/callbacks.py:162-167)
attaches to the contrastive model.  The reference imports it from ``pl_bolts.models.self_supervised.evaluator``; pl_bolts
is not part of this tree, so the class is restated from its public definition (parity with pl_bolts unpinned):

    block_forward = Sequential(Flatten, Dropout(p), Linear(n_input, n_hidden, bias=False), BatchNorm1d(n_hidden),
                               ReLU(inplace=True), Dropout(p), Linear(n_hidden, n_classes, bias=True))

so the state-dict keys are ``block_forward.2.weight``, ``block_forward.3.*`` and ``block_forward.6.{weight,bias}``.

All arithmetic is HIP (csrc/probe.hip).  ``forward(x)`` returns the logits in fp32, in training mode (batch statistics, the
running statistics moved, Philox dropout) or eval mode, in two launches.  ``step(x, target, lr)`` is one whole training
step -- forward, sigmoid + ``nn.BCELoss()``, backward and ``torch.optim.SGD`` -- in three launches; ``evaluate(x, target)``
is the eval-mode forward and loss.  Parameters are fp32 masters; ``compute_dtype`` (attribute, default bf16; the callback
copies the host model's) is the dtype of the activations and of the matrix-instruction operands, fp32 being exact fp32.

Deliberate deviations and notes:
  - ``n_hidden=None`` (pl_bolts' single-Linear form) raises ``NotImplementedError``: the reference never passes it.
  - ``forward`` records no autograd graph: the probe trains through ``step``, whose gradients land in the parameters'
    ``.grad`` (persistent fp32 buffers, allocated zero on the first step).  ``step(accumulate=True)`` adds to them, as
    ``loss.backward()`` does when nobody calls ``zero_grad``.
  - Training-mode dropout draws its masks from the Philox stream of ``functional``: torch's generator stream is not
    reproduced.
  - Shapes outside the kernels' range (``ops.PROBE_LIMITS``) raise ``NotImplementedError``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from .. import functional as F
from .. import ops


class SSLEvaluator(nn.Module):
    def __init__(self, n_input, n_classes, n_hidden=512, p=0.1):
        super().__init__()
        self.n_input = n_input
        self.n_classes = n_classes
        self.n_hidden = n_hidden
        if n_hidden is None:
            raise NotImplementedError("SSLEvaluator(n_hidden=None), pl_bolts' single-Linear probe, is not built: the "
                                      "reference never passes it")
        if n_hidden % 16 or not ops_range_ok(n_input, n_hidden, n_classes):
            raise NotImplementedError(f"SSLEvaluator(n_input={n_input}, n_hidden={n_hidden}, n_classes={n_classes}) is "
                                      f"outside the probe kernels' range ({ops.PROBE_LIMITS})")
        self.block_forward = nn.Sequential(
            nn.Flatten(),
            nn.Dropout(p=p),
            nn.Linear(n_input, n_hidden, bias=False),
            nn.BatchNorm1d(n_hidden),
            nn.ReLU(inplace=True),
            nn.Dropout(p=p),
            nn.Linear(n_hidden, n_classes, bias=True),
        )
        self.compute_dtype = torch.bfloat16

    # ------------------------------------------------------------------ the three launches
    def _desc(self, x: torch.Tensor, training: bool, rng_offset: Optional[int]):
        b = self.block_forward
        x = x.detach().reshape(x.shape[0], -1)
        if x.shape[1] != self.n_input:
            raise ValueError(f"SSLEvaluator: input rows hold {x.shape[1]} elements, expected {self.n_input}")
        x = F.cast(x.contiguous(), self.compute_dtype)
        p = b[1].p if training else 0.0
        if b[5].p != b[1].p:
            raise NotImplementedError("SSLEvaluator: the two dropouts share one p in the probe kernels")
        state, off = None, 0
        if p > 0.0:
            state = F._rng.tensor(x.device)
            off = F._rng.take(x.numel()) if rng_offset is None else int(rng_offset)
            if rng_offset is None:
                F._rng.take(x.shape[0] * self.n_hidden)
        bn = b[3]
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("SSLEvaluator: BatchNorm1d with affine parameters, running statistics and a fixed "
                                      "momentum is what the probe kernels implement")
        return ops.probe_desc(x, b[2].weight.data, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var,
                              bn.num_batches_tracked, b[6].weight.data, b[6].bias.data, training=training, p=p, eps=bn.eps,
                              momentum=bn.momentum, rng_state=state, rng_offset=off)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """-> logits [B, n_classes] fp32 (no autograd graph)."""
        d, keep = self._desc(x, self.training, None)
        ops.probe_fwd(d, keep)
        return ops.probe_logits(d, keep)

    def grads(self):
        """The parameters' ``.grad`` buffers in kernel order (W1, gamma, beta, W2, b2), allocated zero where missing."""
        b = self.block_forward
        out = []
        for prm in (b[2].weight, b[3].weight, b[3].bias, b[6].weight, b[6].bias):
            if prm.grad is None:
                prm.grad = ops.zeros(prm.shape, torch.float32, prm.device)
            out.append(prm.grad)
        return out

    def step(self, x: torch.Tensor, target: torch.Tensor, lr: float, accumulate: bool = True,
             rng_offset: Optional[int] = None, saved: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step in three launches -> (loss 0-dim fp32, probabilities [B, n_classes] fp32), both on the device.
        accumulate: add this step's gradients to ``.grad`` (nobody zeroed it) instead of overwriting it; the update is
        ``p -= lr * p.grad`` either way.  rng_offset: the Philox call offset of the first dropout (default: the next sites
        of ``functional``'s generator).  saved: a dict that receives the step's intermediate tensors (h, z, stats, dlogits)."""
        if not self.training:
            raise RuntimeError("SSLEvaluator.step: the probe trains in training mode (call .train())")
        g_w1, g_g, g_b, g_w2, g_b2 = self.grads()
        d, keep = self._desc(x, True, rng_offset)
        ops.probe_fwd(d, keep)
        loss, prob = ops.probe_loss(d, keep, _target(target, x.shape[0], self.n_classes), g_b2, lr=lr, accumulate=accumulate)
        ops.probe_bwd_step(d, keep, g_w1, g_g, g_b, g_w2)
        if saved is not None:
            saved.update(keep)
        return loss, prob

    def evaluate(self, x: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Eval-mode forward (running statistics, no dropout, nothing moved) and the loss -> (loss, probabilities)."""
        d, keep = self._desc(x, False, None)
        ops.probe_fwd(d, keep)
        return ops.probe_loss(d, keep, _target(target, x.shape[0], self.n_classes))


def ops_range_ok(n_input, n_hidden, n_classes) -> bool:
    """The shape limits of the probe kernels that do not depend on the batch (stated here so that construction needs no
    built library): D <= 4096, H a multiple of 16 up to 2048, C <= 32."""
    return 1 <= n_input <= 4096 and 16 <= n_hidden <= 2048 and n_hidden % 16 == 0 and 1 <= n_classes <= 32


def _target(target: torch.Tensor, B: int, C: int) -> torch.Tensor:
    t = target.detach().reshape(B, C)
    if t.dtype in (torch.bfloat16, torch.float16):
        t = F.cast(t.contiguous(), torch.float32)
    elif t.dtype != torch.float32:
        t = t.to(torch.float32)                   # dtype plumbing of an integer / bool label mask
    return t.contiguous()
