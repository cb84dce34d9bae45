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

``SSLOnlineEval`` (callbacks.py:147-300) is the online probe of the contrastive model: after every training batch it trains
an ``SSLEvaluator`` on the detached embedding (three launches, csrc/probe.hip), after every validation batch it accumulates
the probe's probabilities, and at the end of the validation epoch it logs weighted F1 / recall / precision / average
precision of the binarised predictions at six thresholds, from one launch of integer counts
(``ops.multilabel_sweep_counts``) and float64 ratios on the host.

``AUROC``, ``F1`` and ``ConfusionMatrix`` carry the torchmetrics-0.6 names the reference imports next to
``AveragePrecision`` (frame_transformer.py:8, basicmlp.py:20; scikit-learn's ``confusion_matrix``, callbacks.py:14): AUROC
from one sort and a parallel rank pass over stored rows (``ops.rank_metrics``), F1 and the confusion matrix from integer
counts that reduce over the ranks with one all-reduce (``reduce_counts``).  ``MITEval`` (callbacks.py:85-98) is the accuracy
callback of the MIT runs.
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
ONLINE_THRESHOLDS = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)                # callbacks.py:256
ONLINE_TABLE_THRESHOLD = 0.3                                      # callbacks.py:277
ONLINE_TABLE_ROWS = 20                                            # callbacks.py:287
ONLINE_TARGET_NAMES = ("Action", "Adventure", "Comedy", "Crime", "Documentary", "Drama", "Family", "Fantasy", "History",
                       "Horror", "Music", "Mystery", "Science Fiction", "Thriller", "War")     # callbacks.py:251-252
ONLINE_LR = 0.005                                                 # callbacks.py:167
_ONLINE_FIELDS = ("f1", "recall", "precision", "avg_precision")


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


def _ratio1(num: int, den: int) -> float:
    return num / den if den > 0 else 1.0                          # zero_division=1


def online_scores_from_counts(tp, fp, fn, support, n_rows: int) -> Dict[str, float]:
    """Per-class TP / FP / FN / support of one threshold (integer sequences) over n_rows samples -> what the reference
    logs for it (callbacks.py:258-265): ``f1_score`` / ``recall_score`` / ``precision_score(average="weighted",
    zero_division=1)`` and ``average_precision_score(average="weighted")`` of the BINARISED predictions, in float64.

    A class ratio with a zero denominator is 1; the weights are support / sum(support).  A 0/1 score has one operating
    point besides "everything predicted", so per class with P = support:
        AP = (TP / P) * TP / (TP + FP) + (1 - TP / P) * P / n_rows,
    the first term 0 when nothing is predicted, and AP = 0 for a class without support (its weight is 0 as well)."""
    tp, fp, fn, support = ([int(v) for v in a] for a in (tp, fp, fn, support))
    total = sum(support)
    f1 = rec = prec = ap = 0.0
    for k, P in enumerate(support):
        if P == 0:
            continue                                              # weight 0 (the class's own ratios do not matter)
        w = P / total
        f1 += w * _ratio1(2 * tp[k], 2 * tp[k] + fp[k] + fn[k])
        rec += w * _ratio1(tp[k], tp[k] + fn[k])
        prec += w * _ratio1(tp[k], tp[k] + fp[k])
        r = tp[k] / P
        first = r * tp[k] / (tp[k] + fp[k]) if tp[k] + fp[k] > 0 else 0.0
        ap += w * (first + (1.0 - r) * P / n_rows)
    if total == 0:                                                # no positive label at all: every class ratio is 1 / 0
        return dict(zip(_ONLINE_FIELDS, (float("nan"),) * 4))
    return dict(zip(_ONLINE_FIELDS, (f1, rec, prec, ap)))


def online_scalars_from_counts(counts, support, n_rows: int, thresholds=ONLINE_THRESHOLDS, state: str = "val"
                               ) -> Dict[str, float]:
    """counts [T, 3, C] (TP, FP, FN per class per threshold) and support [C] -> the 4 T scalars under the reference's keys
    ``{state}/online/{f1,recall,precision,avg_precision}@{str(t)}``."""
    c, sup = counts.tolist(), support.tolist()
    if len(c) != len(thresholds):
        raise ValueError(f"{len(c)} count blocks for {len(thresholds)} thresholds")
    out: Dict[str, float] = {}
    for (tp, fp, fn), t in zip(c, thresholds):
        for name, v in online_scores_from_counts(tp, fp, fn, sup, n_rows).items():
            out[f"{state}/online/{name}@{str(t)}"] = v
    return out


def online_scalars(probs: torch.Tensor, labels: torch.Tensor, thresholds=ONLINE_THRESHOLDS, state: str = "val"
                   ) -> Dict[str, float]:
    """probs / labels [N, C] on the device -> the scalars of ``online_scalars_from_counts``: one sweep launch, one
    device->host copy."""
    counts, support = ops.multilabel_sweep_counts(probs, labels, thresholds)
    host = torch.cat((counts.reshape(-1), support)).cpu()
    T, C = counts.shape[0], counts.shape[2]
    return online_scalars_from_counts(host[: T * 3 * C].view(T, 3, C), host[T * 3 * C:], probs.shape[0], thresholds, state)


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


class SSLOnlineEval:
    """callbacks.py:147-300: the MLP probe trained online on the contrastive model's embedding.

    Same constructor as the reference (``drop_p``, ``z_dim``, ``num_classes``, ``model``) plus ``group`` (data parallelism:
    the validation rows of every rank are gathered before the scores are formed) and ``zero_grad``.

    Deliberate deviations and notes:
      - Kept: ``on_train_batch_end`` runs the model's forward in whatever mode the model is in, so in training the
        encoder's BatchNorm running statistics move once more per batch and ``num_batches_tracked`` grows by 1.
      - Kept: the reference never zeroes the probe's gradients, so ``loss.backward()`` accumulates them from step to step
        and every SGD update uses the running sum.  That is the default here (``zero_grad=False``); ``zero_grad=True``
        gives the conventional probe (each update uses its own batch's gradient).
      - The probe step is three HIP launches (forward, loss, backward + SGD); the callback touches no parameter or
        gradient of the model itself.
      - ``running_logits`` / ``running_labels`` stay on the device (the reference moves them to the host), as in
        ``TransformerEval``; the scores come from integer counts of one launch, the ratios are float64 on the host.
      - The truth / guess table covers the first ``min(20, N)`` rows (the reference's fixed ``range(0, 20)`` fails on a
        shorter epoch) and is handed to ``pl_module.logger.experiment.log`` only if such a logger exists (wandb is not
        part of this tree); ``on_shared_end`` returns the scalars and the rows.
      - ``get_representations`` does not ``squeeze()``: ``to_device`` already builds [B, D] rows (and a batch of one row
        keeps its batch dimension)."""

    def __init__(self, drop_p=0.1, z_dim=None, num_classes=None, model="MIT", group: Optional[dist.ProcessGroup] = None,
                 zero_grad: bool = False):
        self.drop_p = drop_p
        self.z_dim = z_dim
        self.num_classes = num_classes
        self.model = model
        self.group = group
        self.zero_grad = zero_grad
        self.lr = ONLINE_LR
        self.optimizer = None

    def on_pretrain_routine_start(self, trainer, pl_module):
        from .models.evaluator import SSLEvaluator
        device = next(pl_module.parameters()).device
        probe = SSLEvaluator(n_input=self.z_dim, n_classes=self.num_classes, p=self.drop_p).to(device)
        probe.compute_dtype = getattr(pl_module, "compute_dtype", torch.float32)
        pl_module.non_linear_evaluator = probe
        # torch.optim.SGD(lr=0.005) holds no state (no momentum, no decay): its step is the tail of the probe's third launch
        self.optimizer = {"lr": self.lr, "momentum": 0.0, "weight_decay": 0.0, "params": list(probe.parameters())}

    def get_representations(self, pl_module, x):
        representations, _ = pl_module(x)
        return representations

    def to_device(self, batch, device):
        """The contrastive collate's ``x_i_experts`` (per sample a list of expert tensors) -> [B, input] rows in one gather
        launch (``rows_input``), labels stacked."""
        from .models.contrastivemodel import rows_input
        rows = [[t.reshape(-1) for t in experts] for experts in batch["x_i_experts"]]
        D = sum(t.numel() for t in rows[0])
        dtype = getattr(self, "_input_dtype", None) or torch.float32
        x = rows_input(rows, D, dtype, device)
        labels = torch.stack([torch.as_tensor(l) for l in batch["label"]]).to(device)
        return x, labels

    def _inputs(self, pl_module, batch):
        device = next(pl_module.parameters()).device
        self._input_dtype = getattr(pl_module, "compute_dtype", torch.float32)
        x, labels = self.to_device(batch, device)
        with torch.no_grad():
            representations = self.get_representations(pl_module, x)
        return representations.detach(), labels

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, data_loader_idx=0):
        representations, labels = self._inputs(pl_module, batch)
        probe = pl_module.non_linear_evaluator
        mlp_loss, _ = probe.step(representations, labels, self.optimizer["lr"], accumulate=not self.zero_grad)
        pl_module.log("train/online/loss", mlp_loss)
        return mlp_loss

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, data_loader_idx=0):
        representations, labels = self._inputs(pl_module, batch)
        with torch.no_grad():
            mlp_loss, probs = pl_module.non_linear_evaluator.evaluate(representations, labels)
        pl_module.log("val/online/loss", mlp_loss)
        pl_module.running_logits.append(probs)
        pl_module.running_labels.append(labels)
        return mlp_loss

    def on_validation_epoch_end(self, trainer, pl_module):
        return self.on_shared_end(pl_module, "val")

    def on_shared_end(self, pl_module, state):
        labels = gather_rows(torch.cat(pl_module.running_labels), self.group)
        probs = gather_rows(torch.cat(pl_module.running_logits), self.group)
        scalars, rows = self._scores(probs, labels, state)
        for k, v in scalars.items():
            pl_module.log(k, v, on_epoch=True)
        pl_module.running_labels = []
        pl_module.running_logits = []
        experiment = getattr(getattr(pl_module, "logger", None), "experiment", None)
        if experiment is not None and callable(getattr(experiment, "log", None)):
            experiment.log({"table": rows})
        return scalars, rows

    def _scores(self, probs, labels, state):
        """-> (the 24 scalars, the truth / guess rows of the first min(20, N) samples at threshold 0.3)."""
        scalars = online_scalars(probs, labels, ONLINE_THRESHOLDS, state)
        n = min(ONLINE_TABLE_ROWS, probs.shape[0])
        head = torch.cat(((labels[:n] != 0).to(torch.uint8), (probs[:n].float() > ONLINE_TABLE_THRESHOLD).to(torch.uint8))).cpu()
        rows = [(self.translate_labels(head[i].tolist()), self.translate_labels(head[n + i].tolist())) for i in range(n)]
        return scalars, rows

    def translate_labels(self, label_vec):
        return [ONLINE_TARGET_NAMES[i] if i < len(ONLINE_TARGET_NAMES) else str(i) for i, l in enumerate(label_vec) if l]


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
        _, _, per_class = ops.average_precision(p, t)
        return list(per_class.unbind(0))

    def reset(self) -> None:
        self.preds, self.target = [], []


def reduce_counts(state: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """Sum an integer state over the ranks with ONE all-reduce (a few C^2 integers instead of ``gather_rows`` of every
    prediction); returns a new tensor and leaves ``state`` as it is, so ``compute()`` can be called again.  Device or CPU
    tensors (gloo); without an initialised process group, or alone in it, the state itself comes back."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return state
    total = state.clone()
    dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    return total


_AUROC_AVERAGES = ("macro", "weighted", "micro", "samples", "none")
_F1_AVERAGES = ("micro", "macro", "weighted", "samples", "none")


def _average(average, allowed, who: str) -> str:
    average = "none" if average is None else average
    if average not in allowed:
        raise ValueError(f"{who}: average must be one of {allowed}, got {average!r}")
    return average


def _num_classes(num_classes, who: str) -> int:
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
        raise ValueError(f"{who}: num_classes must be a positive integer, got {num_classes!r}")
    return num_classes


def _auroc_of(r: "ops.RankMetrics", average: str) -> torch.Tensor:
    if average == "samples":
        return r.samples_sum / r.valid_rows                       # the mean over the rows that have both kinds
    return {"macro": r.macro, "weighted": r.weighted, "micro": r.micro, "none": r.auroc}[average]


class AUROC:
    """Stand-in for ``torchmetrics.AUROC(num_classes=C, average=...)`` on multilabel rows (frame_transformer.py:8,
    :114-115 and the commented log lines :276-343): calling the object with ``(preds, target)`` accumulates a batch on
    the device, ``compute()`` returns a float64 DEVICE scalar (``average="none"``: the [C] vector) without a host
    synchronisation and ``reset()`` clears it.  One descending sort per class and a parallel tie-aware rank pass
    (``ops.rank_metrics``); rank-based, so logits and probabilities give the same value.

    average: ``macro`` / ``weighted`` over the classes that have both kinds, ``micro`` over all N C elements, ``samples``
    over the rows that have both kinds (C <= 64), ``none``.  A class without positives or without negatives is NaN in
    ``none`` and left out of the averages (torchmetrics raises there, which would need a host read)."""

    def __init__(self, num_classes: int, average: Optional[str] = "macro"):
        self.num_classes = _num_classes(num_classes, "AUROC")
        self.average = _average(average, _AUROC_AVERAGES, "AUROC")
        self.preds: List[torch.Tensor] = []
        self.target: List[torch.Tensor] = []

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update(preds, target)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if preds.shape[-1] != self.num_classes or target.shape[-1] != self.num_classes:
            raise ValueError(f"expected {self.num_classes} classes")
        self.preds.append(preds.detach().reshape(-1, self.num_classes))
        self.target.append(target.detach().reshape(-1, self.num_classes))

    def compute(self, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
        if not self.preds:
            raise RuntimeError("AUROC.compute() before any update")
        p = gather_rows(torch.cat(self.preds), group)
        t = gather_rows(torch.cat(self.target), group)
        return _auroc_of(ops.rank_metrics(p, t, micro=self.average == "micro", samples=self.average == "samples"),
                         self.average)

    def reset(self) -> None:
        self.preds, self.target = [], []


def auroc(preds: torch.Tensor, target: torch.Tensor, num_classes: Optional[int] = None, average: Optional[str] = "macro"
          ) -> torch.Tensor:
    """Functional form of ``AUROC``: preds / target [N, C] on the device -> float64 device scalar ([C] for ``none``)."""
    m = AUROC(preds.shape[-1] if num_classes is None else num_classes, average)
    m.update(preds, target)
    return m.compute()


def f1_from_counts(tp: torch.Tensor, fp: torch.Tensor, fn: torch.Tensor, average: str) -> torch.Tensor:
    """Per-class TP / FP / FN (int64 [C], on the host) -> ``f1_score(..., average=average, zero_division=0)`` in float64."""
    tp, fp, fn = tp.double(), fp.double(), fn.double()

    def ratio(num, den):
        return torch.where(den > 0, num / den.clamp(min=1.0), torch.zeros_like(num))

    per = ratio(2 * tp, 2 * tp + fp + fn)
    if average == "none":
        return per
    if average == "micro":
        return ratio(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum())
    if average == "macro":
        return per.mean()
    sup = tp + fn                                                 # weighted
    return ratio((per * sup).sum(), sup.sum())


class _CountMetric:
    """Shared update of ``F1`` and ``ConfusionMatrix``: the state is integer counts on the device, never stored rows --
    ``cm`` int64 [C, C] (+ the skipped rows) for multiclass input, ``counts`` int64 [4, C] (TP / FP / FN / TN) for
    multilabel input.  The mode comes from the target: [N] integers -> multiclass (preds: [N, C] logits, the row's argmax,
    or [N] integers), [N, C] -> multilabel (``preds > threshold``)."""

    def __init__(self, num_classes: int, threshold: float, who: str):
        self.num_classes = _num_classes(num_classes, who)
        self.threshold = float(threshold)
        self._who = who
        self.reset()

    def reset(self) -> None:
        self.mode: Optional[str] = None
        self.cm = self.ignored = self.counts = None

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.update(preds, target)

    def _mode_of(self, preds: torch.Tensor, target: torch.Tensor) -> str:
        C = self.num_classes
        if target.dim() == 1 and not target.is_floating_point():
            if (preds.dim() == 2 and preds.shape[1] != C) or preds.dim() not in (1, 2) or preds.shape[0] != target.shape[0]:
                raise ValueError(f"{self._who}: preds {tuple(preds.shape)} for {target.shape[0]} targets of {C} classes")
            return "multiclass"
        if target.dim() == 2 and tuple(preds.shape) == tuple(target.shape):
            if target.shape[1] != C:
                raise ValueError(f"{self._who}: expected {C} classes, got {target.shape[1]}")
            return "multilabel"
        raise ValueError(f"{self._who}: target {tuple(target.shape)} {target.dtype} with preds {tuple(preds.shape)}: give "
                         "[N] integer targets (multiclass) or [N, C] targets with [N, C] scores (multilabel)")

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        preds, target = preds.detach(), target.detach()
        mode = self._mode_of(preds, target)
        if self.mode not in (None, mode):
            raise ValueError(f"{self._who}: {mode} input after {self.mode} input; reset() first")
        C, dev = self.num_classes, preds.device
        if mode == "multiclass":
            if self.cm is None:
                self.cm, self.ignored = ops.zeros((C, C), torch.int64, dev), ops.zeros((1,), torch.int64, dev)
            ops.confusion_matrix(preds, target, C, self.cm, self.ignored)
        else:
            if self.counts is None:
                self.counts = ops.zeros((4, C), torch.int64, dev)
            ops.multilabel_counts(preds, target, self.threshold, self.counts)
        self.mode = mode

    def _state(self, group) -> torch.Tensor:
        if self.mode is None:
            raise RuntimeError(f"{self._who}.compute() before any update")
        return reduce_counts(self.cm if self.mode == "multiclass" else self.counts, group)


class F1(_CountMetric):
    """Stand-in for ``torchmetrics.F1(num_classes=C, threshold=0.5, average="micro")`` (basicmlp.py:20,
    frame_transformer.py:8): a user assigns ``model.f1 = metrics.F1(22)``.  The state is the integer counts of
    ``_CountMetric`` (under data parallelism one small all-reduce, ``reduce_counts``); ``compute()`` copies them to the host
    once and forms the ratios in float64 there (zero_division = 0, as scikit-learn's ``f1_score``) -> a CPU float64 scalar,
    [C] for ``none``.  ``samples`` is multilabel only: the float64 sum over rows of the per-row F1 (the row sums of
    ``ops.multilabel_report_counts``) and the row count join the state."""

    def __init__(self, num_classes: int, threshold: float = 0.5, average: Optional[str] = "micro"):
        self.average = _average(average, _F1_AVERAGES, "F1")
        super().__init__(num_classes, threshold, "F1")

    def reset(self) -> None:
        super().reset()
        self.row_f1 = None                                        # f64 [2] on the device: sum of the per-row F1, rows

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if self.average == "samples" and self._mode_of(preds, target) != "multilabel":
            raise ValueError("F1: average='samples' is defined for multilabel input only")
        super().update(preds, target)
        if self.average != "samples":
            return
        _, sums = ops.multilabel_report_counts(preds.detach(), target.detach(), self.threshold)
        add = torch.stack((sums[2], torch.full_like(sums[2], float(preds.shape[0]))))
        self.row_f1 = add if self.row_f1 is None else self.row_f1 + add

    def compute(self, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
        state = self._state(group)
        if self.average == "samples":
            s = reduce_counts(self.row_f1, group).cpu()
            return s[0] / s[1]
        state = state.cpu()                                       # the one device->host copy
        if self.mode == "multiclass":
            tp = state.diagonal()
            fp, fn = state.sum(0) - tp, state.sum(1) - tp
        else:
            tp, fp, fn = state[0], state[1], state[2]
        return f1_from_counts(tp, fp, fn, self.average)


class ConfusionMatrix(_CountMetric):
    """Stand-in for ``torchmetrics.ConfusionMatrix(num_classes=C, multilabel=False, threshold=0.5)`` and scikit-learn's
    ``confusion_matrix`` (callbacks.py:14): ``compute()`` returns the int64 DEVICE tensor [C, C] (rows = target, columns =
    prediction), or [C, 2, 2] = [[TN, FP], [FN, TP]] per class for multilabel input (``multilabel_confusion_matrix``).
    ``ignored`` counts the rows whose target was outside [0, C)."""

    def __init__(self, num_classes: int, multilabel: bool = False, threshold: float = 0.5):
        self.multilabel = bool(multilabel)
        super().__init__(num_classes, threshold, "ConfusionMatrix")

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        mode = self._mode_of(preds.detach(), target.detach())
        if (mode == "multilabel") != self.multilabel:
            raise ValueError(f"ConfusionMatrix(multilabel={self.multilabel}) got {mode} input")
        super().update(preds, target)

    def compute(self, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
        state = self._state(group)
        if self.mode == "multiclass":
            return state
        tp, fp, fn, tn = state.unbind(0)
        return torch.stack((torch.stack((tn, fp), 1), torch.stack((fn, tp), 1)), 1)


def f1(preds: torch.Tensor, target: torch.Tensor, num_classes: int, threshold: float = 0.5,
       average: Optional[str] = "micro") -> torch.Tensor:
    """Functional form of ``F1``."""
    m = F1(num_classes, threshold, average)
    m.update(preds, target)
    return m.compute()


def confusion_matrix(preds: torch.Tensor, target: torch.Tensor, num_classes: int, multilabel: bool = False,
                     threshold: float = 0.5) -> torch.Tensor:
    """Functional form of ``ConfusionMatrix``."""
    m = ConfusionMatrix(num_classes, multilabel, threshold)
    m.update(preds, target)
    return m.compute()


class MITEval:
    """callbacks.py:85-98, the accuracy callback src/main.py:46-50 attaches to every MIT run: at the end of a validation epoch
    ``acc = sum(running_logits == running_labels) / len(running_labels)`` is logged under ``"val/accuracy/epoch"`` and the
    accumulators are reset.  The comparison is counted on the device (``ops.count_equal``), under data parallelism the two
    integers (matches, rows) are summed over the ranks (``reduce_counts``), and one device->host copy fetches them for the
    logged scalar.  ``best_acc`` is kept as the reference keeps it (its update is commented out there); the reference's
    ``print`` of element 0 is not reproduced."""

    def __init__(self, group: Optional[dist.ProcessGroup] = None):
        self.best_acc = 0
        self.group = group

    def on_validation_epoch_end(self, trainer, pl_module) -> float:
        labels = torch.cat(pl_module.running_labels)
        preds = torch.cat(pl_module.running_logits)
        state = torch.cat((ops.count_equal(preds, labels),
                           torch.tensor([labels.shape[0]], dtype=torch.int64).to(labels.device)))
        matches, rows = reduce_counts(state, self.group).cpu().tolist()
        acc = matches / (rows * 1.0)
        pl_module.log("val/accuracy/epoch", acc, on_step=False, on_epoch=True)
        pl_module.running_labels = []
        pl_module.running_logits = []
        return acc


class CosineSimilarity:
    """``nn.CosineSimilarity(dim=1)`` for logging (frame_transformer.py:121,257); no gradient."""

    def __init__(self, dim: int = 1, eps: float = 1e-8):
        if dim != 1:
            raise ValueError("only dim=1 (rows of a [B, C] pair) is used by the reference")
        self.eps = eps

    def __call__(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return ops.cosine_rows(a, b, self.eps)
