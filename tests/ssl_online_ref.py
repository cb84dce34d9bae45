"""Torch-CPU restatement, in float64, of the online probe (SSLOnlineEval's SSLEvaluator step, src/callbacks/callbacks.py:
147-241) written from its documented semantics: Dropout -> Linear (no bias) -> BatchNorm1d -> ReLU -> Dropout -> Linear ->
sigmoid -> nn.BCELoss() (mean, logs clamped at -100) and torch.optim.SGD; and numpy restatements of the counts and scores of
its validation epoch.  The yardstick of tests/test_gpu_ssl_online.py."""
from __future__ import annotations

import numpy as np
import torch

KEYS = ("block_forward.2.weight", "block_forward.3.weight", "block_forward.3.bias", "block_forward.6.weight",
        "block_forward.6.bias")


def params64(module):
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in module.named_parameters()}


def stats64(module):
    bn = module.block_forward[3]
    return [bn.running_mean.detach().cpu().double().clone(), bn.running_var.detach().cpu().double().clone()]


def forward(P, x, stats, training, mask1=None, mask2=None, p=0.0, eps=1e-5, momentum=0.1):
    """-> (h, logits).  mask1 [B, D] / mask2 [B, H]: the keep masks of the two dropouts (None: keep everything)."""
    if mask1 is not None:
        x = x * mask1 / (1 - p)
    z = x @ P[KEYS[0]].T
    if training:
        mean, var = z.mean(0), z.var(0, unbiased=False)
        with torch.no_grad():
            n = z.shape[0]
            stats[0].mul_(1 - momentum).add_(momentum * mean.detach())
            stats[1].mul_(1 - momentum).add_(momentum * var.detach() * n / (n - 1))
    else:
        mean, var = stats[0], stats[1]
    h = torch.relu((z - mean) / torch.sqrt(var + eps) * P[KEYS[1]] + P[KEYS[2]])
    if mask2 is not None:
        h = h * mask2 / (1 - p)
    return h, h @ P[KEYS[3]].T + P[KEYS[4]]


def bce(prob, y):
    return -(y * torch.log(prob).clamp(min=-100) + (1 - y) * torch.log1p(-prob).clamp(min=-100)).mean()


def step(P, x, y, stats, **kw):
    """One training step's forward and backward -> (loss, prob, h, {key: gradient}); P is not updated."""
    for v in P.values():
        v.grad = None
    h, logits = forward(P, x, stats, True, **kw)
    prob = torch.sigmoid(logits)
    loss = bce(prob, y)
    loss.backward()
    return loss.detach(), prob.detach(), h.detach(), {k: P[k].grad.clone() for k in KEYS}


def sweep_counts(probs, labels, thresholds):
    """-> (counts int64 [T, 3, C]: TP / FP / FN of probs > t, compared in float32; support int64 [C])."""
    y = labels.astype(np.int64)
    out = []
    for t in thresholds:
        pr = (probs.astype(np.float32) > np.float32(t)).astype(np.int64)
        out.append(np.stack([(pr & y).sum(0), (pr & (1 - y)).sum(0), ((1 - pr) & y).sum(0)]))
    return np.stack(out).astype(np.int64), y.sum(0).astype(np.int64)


def sklearn_scalars(probs, labels, thresholds, state="val"):
    """The reference's on_shared_end loop through scikit-learn itself (callbacks.py:257-274)."""
    import warnings
    from sklearn.metrics import average_precision_score, f1_score, precision_score, recall_score
    y = labels.astype(int)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t in thresholds:
            pr = (probs.astype(np.float32) > np.float32(t)).astype(int)
            out[f"{state}/online/f1@{str(t)}"] = float(f1_score(y, pr, average="weighted", zero_division=1))
            out[f"{state}/online/recall@{str(t)}"] = float(recall_score(y, pr, average="weighted", zero_division=1))
            out[f"{state}/online/precision@{str(t)}"] = float(precision_score(y, pr, average="weighted", zero_division=1))
            out[f"{state}/online/avg_precision@{str(t)}"] = float(average_precision_score(y, pr, average="weighted"))
    return out
