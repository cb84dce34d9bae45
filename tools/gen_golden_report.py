#!/usr/bin/env python3
"""Writes tests/golden/test_report.npz: the test epoch's classification_report (TransformerEval.on_test_epoch_end, the
reference's src/callbacks/callbacks.py:67-82) through scikit-learn itself, at threshold 0.3 on multilabel rows.

N = 97 rows x 19 classes of random probabilities and labels, with rows that have no positive label, a class with no
support, a class that is never predicted and a row that is neither labelled nor predicted, so that every zero_division
branch is taken.  Stored: the inputs, sklearn's per-class precision / recall / F1 / support (rows of `per_class`) and the
four averages (rows of `averages`, in the order of AVERAGES), plus the integer counts behind them.

    python tools/gen_golden_report.py
"""
from __future__ import annotations

import os
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "test_report.npz")
SEED = 2024
THRESHOLD = 0.3
AVERAGES = ("micro avg", "macro avg", "weighted avg", "samples avg")
FIELDS = ("precision", "recall", "f1-score", "support")


def main() -> None:
    from sklearn.metrics import classification_report
    rng = np.random.default_rng(SEED)
    N, C = 97, 19
    y = (rng.random((N, C)) < 0.2).astype(np.uint8)
    p = rng.random((N, C)).astype(np.float32)
    p[np.abs(p - THRESHOLD) < 1e-4] += 1e-3          # no score within rounding of the threshold
    y[:, 14] = 0                                     # a class without support (TVMovie is rare)
    p[:, 5] = np.minimum(p[:, 5], 0.25)              # a class that is never predicted
    y[[3, 40, 77], :] = 0                            # rows without a positive label
    p[40, :] = 0.1                                   # ... one of them also without a prediction
    pred = (p > np.float32(THRESHOLD)).astype(int)
    names = [f"c{i}" for i in range(C)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = classification_report(y.astype(int), pred, target_names=names, output_dict=True)
    per_class = np.array([[rep[n][f] for f in FIELDS] for n in names], dtype=np.float64)
    averages = np.array([[rep[a][f] for f in FIELDS] for a in AVERAGES], dtype=np.float64)
    counts = np.stack([(pred & y).sum(0), (pred & (1 - y)).sum(0), ((1 - pred) & y).sum(0), y.sum(0)]).astype(np.int64)
    np.savez_compressed(OUT, probs=p, labels=y, threshold=np.array(THRESHOLD), per_class=per_class, averages=averages,
                        counts=counts)
    print(f"test_report: {OUT}; samples avg f1 {averages[3, 2]:.6f}, micro f1 {averages[0, 2]:.6f}")


if __name__ == "__main__":
    main()
