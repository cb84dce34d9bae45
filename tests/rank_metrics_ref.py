"""numpy restatement of the rank metrics and counts of csrc/eval_metrics.hip (test infrastructure, like tests/lars_ref.py).

A tie group is a maximal run of equal scores of a column sorted descending; element i ends a group when it is the last one
or s[i+1] != s[i] (-0.0 == +0.0).  With tp the inclusive count of positives, P the positives, Nn = N - P, and per group
g = [b, e]: pos_g = tp[e] - tp[b-1], neg_g = (e - b + 1) - pos_g,

    2U    = sum_g neg_g (2 tp[b-1] + pos_g)            (Python / int64 integers)
    AUROC = 2U / (2 P Nn)                              (float64; NaN without both kinds)
    AP    = sum_g (pos_g / P) (tp[e] / (e + 1))        (float64; 0 without positives)

The counts (confusion matrix, multilabel TP / FP / FN / TN) and the ratios formed from them (F1 under every average with
zero_division=0, accuracy) follow scikit-learn's definitions."""
import numpy as np


def column(scores, labels):
    """One column -> (two_u int, positives int, auroc float64, ap float64)."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    l = (np.asarray(labels).reshape(-1) != 0).astype(np.int64)
    n = s.shape[0]
    order = np.argsort(-s.astype(np.float64), kind="stable")
    s, l = s[order], l[order]
    tp = np.cumsum(l)
    end = np.ones(n, dtype=bool)
    end[:-1] = s[1:] != s[:-1]
    e = np.nonzero(end)[0]
    tp_e = tp[e]
    tp_b = np.concatenate(([0], tp_e[:-1]))
    size = np.diff(np.concatenate(([-1], e)))
    pos = tp_e - tp_b
    neg = size - pos
    two_u = int(np.sum(neg * (2 * tp_b + pos)))
    P = int(tp[-1])
    Nn = n - P
    auroc = two_u / (2.0 * P * Nn) if P > 0 and Nn > 0 else float("nan")
    ap = float(np.sum((pos / float(P)) * (tp_e / (e + 1.0)))) if P > 0 else 0.0
    return two_u, P, auroc, ap


def rank_metrics(probs, labels, micro=True, samples=True):
    """probs [N, C] (compared as float32), labels [N, C] -> dict of what dvt_rank_metrics writes."""
    probs = np.asarray(probs, dtype=np.float32)
    lab = np.asarray(labels) != 0
    N, C = probs.shape
    cols = [column(probs[:, c], lab[:, c]) for c in range(C)]
    two_u = np.array([c[0] for c in cols], dtype=np.int64)
    positives = np.array([c[1] for c in cols], dtype=np.int64)
    auroc = np.array([c[2] for c in cols], dtype=np.float64)
    ap = np.array([c[3] for c in cols], dtype=np.float64)
    valid = (positives > 0) & (positives < N)
    out = dict(two_u=two_u, positives=positives, auroc=auroc, ap=ap, valid_classes=int(valid.sum()))
    out["macro"] = float(np.mean(auroc[valid])) if valid.any() else float("nan")
    out["weighted"] = (float(np.sum(auroc[valid] * positives[valid]) / np.sum(positives[valid])) if valid.any()
                       else float("nan"))
    if micro:
        u, p, a, _ = column(probs.reshape(-1), lab.reshape(-1))
        out.update(micro=a, micro_two_u=u, micro_positives=p)
    if samples:
        a = rows_auroc(probs, lab)
        ok = ~np.isnan(a)
        out["samples_sum"] = float(np.sum(a[ok])) if ok.any() else 0.0
        out["valid_rows"] = int(ok.sum())
    return out


def rows_auroc(probs, labels):
    """AUROC of every row over its C class scores (NaN for a row without both kinds): the per-element form of 2U, every
    negative contributing S + G -- the positives before its tie group plus the positives through the end of its group --
    over all rows at once."""
    s = np.asarray(probs, dtype=np.float32)
    l = (np.asarray(labels) != 0).astype(np.int64)
    N, C = s.shape
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")
    s, l = np.take_along_axis(s, order, 1), np.take_along_axis(l, order, 1)
    tp = np.cumsum(l, axis=1)
    end = np.ones((N, C), dtype=bool)
    end[:, :-1] = s[:, 1:] != s[:, :-1]
    at_end = np.where(end, tp, 0)
    S = np.concatenate((np.zeros((N, 1), dtype=np.int64), np.maximum.accumulate(at_end, axis=1)[:, :-1]), axis=1)
    G = np.minimum.accumulate(np.where(end, tp, C + 1)[:, ::-1], axis=1)[:, ::-1]
    two_u = np.sum((1 - l) * (S + G), axis=1)
    P = tp[:, -1]
    ok = (P > 0) & (P < C)
    return np.where(ok, two_u / np.where(ok, 2.0 * P * (C - P), 1.0), np.nan)


def argmax_lowest(logits):
    """Row argmax, the lowest index among equal maxima (numpy's rule)."""
    return np.argmax(np.asarray(logits, dtype=np.float32), axis=1).astype(np.int64)


def confusion_matrix(preds, target, C):
    """-> (cm int64 [C, C] with rows = target and columns = prediction, number of skipped rows)."""
    preds, target = np.asarray(preds, dtype=np.int64), np.asarray(target, dtype=np.int64)
    ok = (target >= 0) & (target < C) & (preds >= 0) & (preds < C)
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (target[ok], preds[ok]), 1)
    return cm, int((~ok).sum())


def multilabel_counts(probs, labels, threshold):
    """-> int64 [4, C]: TP, FP, FN, TN of ``probs > threshold`` (strict, float32)."""
    p = np.asarray(probs, dtype=np.float32) > np.float32(threshold)
    l = np.asarray(labels) != 0
    return np.stack([(p & l).sum(0), (p & ~l).sum(0), (~p & l).sum(0), (~p & ~l).sum(0)]).astype(np.int64)


def _div(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)        # zero_division=0


def f1_from_counts(tp, fp, fn, average):
    """Per-class TP / FP / FN -> f1_score(..., average=average, zero_division=0); average in micro / macro / weighted /
    none.  (Multiclass: TP = diag(cm), FP = column sums - TP, FN = row sums - TP.)"""
    tp, fp, fn = (np.asarray(a, dtype=np.int64) for a in (tp, fp, fn))
    per = _div(2 * tp, 2 * tp + fp + fn)
    if average == "none":
        return per
    if average == "micro":
        return float(_div(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum()))
    if average == "macro":
        return float(per.mean())
    if average == "weighted":
        sup = tp + fn
        return float(_div(np.sum(per * sup), sup.sum()))
    raise ValueError(average)


def f1_samples(pred_mask, labels):
    """Multilabel "samples" F1: the mean over rows of 2 |P & T| / (|P| + |T|), 0 where both are empty."""
    p, l = np.asarray(pred_mask) != 0, np.asarray(labels) != 0
    return float(np.mean(_div(2 * (p & l).sum(1), p.sum(1) + l.sum(1))))


def multilabel_confusion(counts):
    """[4, C] TP / FP / FN / TN -> [C, 2, 2] in scikit-learn's layout [[TN, FP], [FN, TP]]."""
    tp, fp, fn, tn = np.asarray(counts, dtype=np.int64)
    return np.stack([np.stack([tn, fp], 1), np.stack([fn, tp], 1)], 1)


def accuracy(preds, target):
    preds, target = np.asarray(preds), np.asarray(target)
    return float(np.sum(preds == target)) / preds.shape[0]
