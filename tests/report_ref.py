"""numpy restatement of scikit-learn's multilabel ``classification_report`` (zero_division=0), the test epoch's report
(callbacks.py:67-82).  Independent of the package: the GPU tests hold the device reduction against it."""
from __future__ import annotations

import numpy as np

AVERAGES = ("micro avg", "macro avg", "weighted avg", "samples avg")
FIELDS = ("precision", "recall", "f1-score", "support")


def _div(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def counts(probs, labels, threshold):
    """-> int64 [4, C]: TP, FP, FN, support per class."""
    p = (np.asarray(probs, dtype=np.float32) > np.float32(threshold)).astype(np.int64)
    y = (np.asarray(labels) != 0).astype(np.int64)
    return np.stack([(p & y).sum(0), (p & (1 - y)).sum(0), ((1 - p) & y).sum(0), y.sum(0)])


def report_arrays(probs, labels, threshold):
    """-> (per_class [C, 4], averages [4, 4]) with the columns of FIELDS and the rows of AVERAGES."""
    p = (np.asarray(probs, dtype=np.float32) > np.float32(threshold)).astype(np.int64)
    y = (np.asarray(labels) != 0).astype(np.int64)
    tp, fp, fn, sup = counts(probs, labels, threshold)
    prec, rec, f1 = _div(tp, tp + fp), _div(tp, tp + fn), _div(2 * tp, 2 * tp + fp + fn)
    per_class = np.stack([prec, rec, f1, sup.astype(np.float64)], 1)
    total = float(sup.sum())
    TP, FP, FN = tp.sum(), fp.sum(), fn.sum()
    micro = [float(_div(TP, TP + FP)), float(_div(TP, TP + FN)), float(_div(2 * TP, 2 * TP + FP + FN)), total]
    macro = [prec.mean(), rec.mean(), f1.mean(), total]
    weighted = [float(_div((v * sup).sum(), total)) for v in (prec, rec, f1)] + [total]
    rtp, rp, rt = (p & y).sum(1), p.sum(1), y.sum(1)
    samples = [_div(rtp, rp).mean(), _div(rtp, rt).mean(), _div(2 * rtp, rp + rt).mean(), total]
    return per_class, np.array([micro, macro, weighted, samples], dtype=np.float64)


def report_dict(probs, labels, threshold, names):
    per_class, averages = report_arrays(probs, labels, threshold)
    out = {n: dict(zip(FIELDS, map(float, row))) for n, row in zip(names, per_class)}
    out.update({a: dict(zip(FIELDS, map(float, row))) for a, row in zip(AVERAGES, averages)})
    return out
