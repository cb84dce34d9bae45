"""Write tests/golden/rank_metrics.npz: small inputs and what scikit-learn computes from them.

    python tools/gen_golden_rank_metrics.py

Needs scikit-learn (the tests do not: they read the fixture).  Rank cases: roc_auc_score under every average and
average_precision_score per class; count cases: f1_score under every average (zero_division=0), confusion_matrix,
multilabel_confusion_matrix, accuracy_score.  Labels are Bernoulli(0.3) with row 0 all ones and row 1 all zeros, so every
class has both kinds; the "samples" average is taken over the rows that have both kinds (scikit-learn raises on the others),
and the number of those rows is stored next to it."""
import os

import numpy as np
from sklearn import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rank_metrics.npz")

# name -> (N, C, levels; 0 = continuous)
RANK_CASES = {"cont_1025x19": (1025, 19, 0), "cont_64x1": (64, 1, 0), "q1_130x5": (130, 5, 1), "q2_255x19": (255, 19, 2),
              "q4_257x7": (257, 7, 4), "q8_257x19": (257, 19, 8), "q16_300x15": (300, 15, 16)}
# name -> (N, C)
MULTICLASS_CASES = {"mc_301x22": (301, 22), "mc_65x2": (65, 2), "mc_120x305": (120, 305)}
MULTILABEL_CASES = {"ml_653x19": (653, 19), "ml_97x15": (97, 15), "ml_33x1": (33, 1)}
THRESHOLD = 0.5


def make_labels(rng, N, C):
    lab = (rng.random((N, C)) < 0.3).astype(np.uint8)
    if N >= 2:
        lab[0], lab[1] = 1, 0
    return lab


def make_scores(rng, N, C, levels):
    x = rng.random((N, C)).astype(np.float32)
    if levels:
        x = (np.floor(x * levels) / levels).astype(np.float32)
    return x


def rank_case(rng, N, C, levels, equal_column=False):
    probs, lab = make_scores(rng, N, C, levels), make_labels(rng, N, C)
    if equal_column:
        probs[:, C // 2] = 0.25
    p64 = probs.astype(np.float64)
    out = {"probs": probs, "labels": lab}
    out["auroc"] = np.array([M.roc_auc_score(lab[:, c], p64[:, c]) for c in range(C)])
    out["ap"] = np.array([M.average_precision_score(lab[:, c], p64[:, c]) for c in range(C)])
    if C > 1:
        for avg in ("macro", "weighted", "micro"):
            out["auroc_" + avg] = np.float64(M.roc_auc_score(lab, p64, average=avg))
            out["ap_" + avg] = np.float64(M.average_precision_score(lab, p64, average=avg))
        ok = (lab.sum(1) > 0) & (lab.sum(1) < C)
        out["auroc_samples"] = np.float64(M.roc_auc_score(lab[ok], p64[ok], average="samples"))
        out["valid_rows"] = np.int64(ok.sum())
    return out


def multiclass_case(rng, N, C):
    logits = rng.standard_normal((N, C)).astype(np.float32)
    target = rng.integers(0, C, N).astype(np.int64)
    logits[np.arange(N), target] += 1.0                       # better than chance
    logits[3] = logits[3, 0]                                  # a row of equal maxima: the lowest index wins
    if N > 40:
        logits[40, 1:4] = logits[40].max() + 1.0              # a three-way tie away from index 0
    pred = np.argmax(logits, axis=1)
    labels = np.arange(C)
    out = {"logits": logits, "target": target, "pred": pred.astype(np.int64)}
    for avg in ("micro", "macro", "weighted"):
        out["f1_" + avg] = np.float64(M.f1_score(target, pred, labels=labels, average=avg, zero_division=0))
    out["f1_none"] = M.f1_score(target, pred, labels=labels, average=None, zero_division=0)
    out["cm"] = M.confusion_matrix(target, pred, labels=labels).astype(np.int64)
    out["accuracy"] = np.float64(M.accuracy_score(target, pred))
    return out


def multilabel_case(rng, N, C):
    probs, lab = make_scores(rng, N, C, 0), make_labels(rng, N, C)
    probs[5 % N, 0] = THRESHOLD                                # equal to the threshold: strict > leaves it negative
    pred = (probs > np.float32(THRESHOLD)).astype(np.uint8)
    out = {"probs": probs, "labels": lab}
    y, p = (lab, pred) if C > 1 else (lab[:, 0], pred[:, 0])
    for avg in ("micro", "macro", "weighted") + (("samples",) if C > 1 else ()):
        kw = {} if C > 1 else {"labels": [1]}
        out["f1_" + avg] = np.float64(M.f1_score(y, p, average=avg, zero_division=0, **kw))
    out["f1_none"] = np.atleast_1d(M.f1_score(y, p, average=None, zero_division=0, **({} if C > 1 else {"labels": [1]})))
    out["mcm"] = (M.multilabel_confusion_matrix(lab, pred) if C > 1
                  else M.confusion_matrix(y, p, labels=[0, 1])[None]).astype(np.int64)
    return out


def main():
    rng = np.random.default_rng(20261019)
    blob = {}
    for name, (N, C, levels) in RANK_CASES.items():
        for k, v in rank_case(rng, N, C, levels).items():
            blob[f"{name}/{k}"] = v
    for k, v in rank_case(rng, 257, 6, 0, equal_column=True).items():
        blob[f"equalcol_257x6/{k}"] = v
    for name, (N, C) in MULTICLASS_CASES.items():
        for k, v in multiclass_case(rng, N, C).items():
            blob[f"{name}/{k}"] = v
    for name, (N, C) in MULTILABEL_CASES.items():
        for k, v in multilabel_case(rng, N, C).items():
            blob[f"{name}/{k}"] = v
    blob["threshold"] = np.float32(THRESHOLD)
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT}: {len(blob)} arrays, {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
