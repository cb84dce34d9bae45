"""Evaluation-side reductions on the device and the callback that consumes them.

Mirror of ``TransformerEval`` (src/callbacks/callbacks.py:27-66): at the end of a validation epoch the
accumulated ``pl_module.running_logits`` / ``running_labels`` are reduced to the samples-F1 threshold sweep and
the two average-precision scores, logged under the reference's keys, and the accumulators are reset.  The
reference moves everything to the host and calls scikit-learn; here the tensors stay in HBM, and under data
parallelism every rank first all-gathers the other ranks' accumulators (the reference is single-GPU).

The test epoch (``on_test_epoch_end``, callbacks.py:67-82) prints scikit-learn's multilabel ``classification_report`` at
threshold 0.3: here the counts behind it (per-class TP / FP / FN / support, the per-row ratio sums of the "samples"
average) come from one device reduction (``ops.multilabel_report_counts``) and the ratios of those few integers are
formed in float64 on the host.
"""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import ops

THRESHOLDS = (0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)          # callbacks.py:38
REPORT_THRESHOLD = 0.3                                            # callbacks.py:80
TARGET_NAMES = ("Action", "Animation", "Adventure", "Comedy", "Crime", "Documentary", "Drama", "Family", "Fantasy",
                "History", "Horror", "Music", "Romance", "Mystery", "TVMovie", "ScienceFiction", "Thriller", "War",
                "Western")                                        # callbacks.py:70-71
_REPORT_FIELDS = ("precision", "recall", "f1-score", "support")


def gather_rows(t: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """Concatenate every rank's rows (ranks may hold different row counts)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return t
    world = dist.get_world_size(group)
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c.item()) for c in counts]
    cap = max(counts)
    pad = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[: t.shape[0]] = t
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0)


def evaluate(probs: torch.Tensor, labels: torch.Tensor, thresholds=THRESHOLDS) -> Dict[str, float]:
    """probs [N, C] (sigmoid outputs), labels [N, C] -> the reference's logged scalars."""
    f1 = ops.f1_samples(probs, labels, thresholds)
    ap_s, ap_w, _ = ops.average_precision(probs, labels)
    host = torch.cat((f1, ap_s, ap_w)).cpu()                      # one device->host copy per epoch
    out = {f"val/online/f1@{str(t)}": float(host[i]) for i, t in enumerate(thresholds)}
    out["sklearn apr"] = float(host[len(thresholds)])
    out["sklearn apr weighted"] = float(host[len(thresholds) + 1])
    return out


def _div(num: float, den: float) -> float:
    return num / den if den > 0 else 0.0                          # zero_division=0 (sklearn's default, "warn" -> 0)


def report_from_counts(counts, row_sums, n_rows: int, target_names: Sequence[str]) -> Dict[str, Dict[str, float]]:
    """counts [4, C] (TP, FP, FN, support per class) and row_sums [3] (sums over rows of the per-row precision / recall /
    F1) -> the dict of ``classification_report(..., output_dict=True)`` for multilabel indicator targets."""
    c = [[int(v) for v in row] for row in counts.tolist()]
    tp, fp, fn, sup = c
    C = len(tp)
    if len(target_names) != C:
        raise ValueError(f"{len(target_names)} target names for {C} classes")
    out: Dict[str, Dict[str, float]] = {}
    prf = []
    for k in range(C):
        p, r = _div(tp[k], tp[k] + fp[k]), _div(tp[k], tp[k] + fn[k])
        f = _div(2 * tp[k], 2 * tp[k] + fp[k] + fn[k])
        prf.append((p, r, f))
        out[target_names[k]] = dict(zip(_REPORT_FIELDS, (p, r, f, float(sup[k]))))
    total = float(sum(sup))
    TP, FP, FN = sum(tp), sum(fp), sum(fn)
    out["micro avg"] = dict(zip(_REPORT_FIELDS, (_div(TP, TP + FP), _div(TP, TP + FN), _div(2 * TP, 2 * TP + FP + FN), total)))
    out["macro avg"] = dict(zip(_REPORT_FIELDS, tuple(sum(v[j] for v in prf) / C for j in range(3)) + (total,)))
    out["weighted avg"] = dict(zip(_REPORT_FIELDS, tuple(_div(sum(v[j] * sup[k] for k, v in enumerate(prf)), total)
                                                         for j in range(3)) + (total,)))
    rs = [float(v) for v in row_sums.tolist()]
    out["samples avg"] = dict(zip(_REPORT_FIELDS, tuple(v / n_rows for v in rs) + (total,)))
    return out


def classification_report(probs: torch.Tensor, labels: torch.Tensor, threshold: float = REPORT_THRESHOLD,
                          target_names: Sequence[str] = TARGET_NAMES) -> Dict[str, Dict[str, float]]:
    """``sklearn.metrics.classification_report(labels, probs > threshold, target_names=..., output_dict=True)`` for
    multilabel rows probs / labels [N, C] on the device; one device->host copy of the counts."""
    counts, sums = ops.multilabel_report_counts(probs, labels, threshold)
    return report_from_counts(counts.cpu(), sums.cpu(), probs.shape[0], target_names)


def format_report(report: Dict[str, Dict[str, float]], digits: int = 2) -> str:
    """The text form sklearn prints (``classification_report`` without ``output_dict``)."""
    heads = ("precision", "recall", "f1-score", "support")
    width = max(len(k) for k in report)
    head_fmt = "{:>{width}s} " + " {:>9}" * len(heads)
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    text = head_fmt.format("", *heads, width=width) + "\n\n"
    for name, v in report.items():
        if name == "micro avg":
            text += "\n"
        text += row_fmt.format(name, v["precision"], v["recall"], v["f1-score"], int(round(v["support"])), width=width,
                               digits=digits)
    return text


class TransformerEval:
    """callbacks.py:27-82: ``on_validation_epoch_end`` (same log keys, same accumulator reset) and ``on_test_epoch_end``.

    dump_dir: where the test epoch pickles its gathered accumulators (rank 0), as the reference does into the working
    directory (files ``labels`` and ``logits``); None writes nothing."""

    def __init__(self, group: Optional[dist.ProcessGroup] = None, dump_dir: Optional[str] = None):
        self.group = group
        self.dump_dir = dump_dir

    def on_validation_epoch_end(self, trainer, pl_module) -> Dict[str, float]:
        labels = gather_rows(torch.cat(pl_module.running_labels), self.group)
        probs = gather_rows(torch.cat(pl_module.running_logits), self.group)
        scalars = evaluate(probs, labels)
        for k, v in scalars.items():
            pl_module.log(k, v)
        pl_module.running_labels = []
        pl_module.running_logits = []
        return scalars

    def on_test_epoch_end(self, trainer, pl_module) -> Dict[str, Dict[str, float]]:
        """callbacks.py:67-82: the multilabel ``classification_report`` of every rank's accumulated rows at threshold 0.3,
        keyed by the reference's 19 target names, as sklearn's ``output_dict=True`` gives it; the text form is printed on
        rank 0 and the accumulators are reset.

        Deviation: the reference pickles ``running_labels`` into both of its files; with ``dump_dir`` set, ``logits`` here
        holds the accumulated probabilities (``running_logits``), ``labels`` the labels (CPU tensors)."""
        labels = gather_rows(torch.cat(pl_module.running_labels), self.group)
        probs = gather_rows(torch.cat(pl_module.running_logits), self.group)
        C = probs.shape[1]
        names = TARGET_NAMES if C == len(TARGET_NAMES) else tuple(str(k) for k in range(C))
        report = classification_report(probs, labels, REPORT_THRESHOLD, names)
        rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank(self.group) == 0
        if rank0:
            if self.dump_dir is not None:
                os.makedirs(self.dump_dir, exist_ok=True)
                with open(os.path.join(self.dump_dir, "labels"), "wb") as fp:
                    pickle.dump(labels.cpu(), fp)
                with open(os.path.join(self.dump_dir, "logits"), "wb") as fp:
                    pickle.dump(probs.cpu(), fp)
            print(format_report(report))
        pl_module.running_labels = []
        pl_module.running_logits = []
        return report


class AveragePrecision:
    """Stand-in for ``torchmetrics.AveragePrecision(num_classes=C)`` (frame_transformer.py:114,118,277,335): calling the
    object with ``(preds, target)`` accumulates a batch on the device, ``compute()`` returns the per-class average
    precision (one-vs-rest, a list of C scalars like torchmetrics 0.6) and ``reset()`` clears it.  Average precision is
    rank-based, so logits and probabilities give the same value."""

    def __init__(self, num_classes: int):
        self.num_classes = num_classes
        self.preds: List[torch.Tensor] = []
        self.target: List[torch.Tensor] = []

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update(preds, target)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if preds.shape[-1] != self.num_classes:
            raise ValueError(f"expected {self.num_classes} classes")
        self.preds.append(preds.detach().reshape(-1, self.num_classes))
        self.target.append(target.detach().reshape(-1, self.num_classes))

    def compute(self, group: Optional[dist.ProcessGroup] = None) -> List[torch.Tensor]:
        if not self.preds:
            raise RuntimeError("AveragePrecision.compute() before any update")
        p = gather_rows(torch.cat(self.preds), group)
        t = gather_rows(torch.cat(self.target), group)
        _, _, per_class = ops.average_precision(p.float() if p.dtype != torch.float32 else p, t)
        return list(per_class.unbind(0))

    def reset(self) -> None:
        self.preds, self.target = [], []


class CosineSimilarity:
    """``nn.CosineSimilarity(dim=1)`` for logging (frame_transformer.py:121,257); no gradient."""

    def __init__(self, dim: int = 1, eps: float = 1e-8):
        if dim != 1:
            raise ValueError("only dim=1 (rows of a [B, C] pair) is used by the reference")
        self.eps = eps

    def __call__(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return ops.cosine_rows(a, b, self.eps)
