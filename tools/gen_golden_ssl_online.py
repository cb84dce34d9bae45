#!/usr/bin/env python3
"""Writes tests/golden/ssl_online.npz: the validation-epoch scores of SSLOnlineEval.on_shared_end (the reference's
src/callbacks/callbacks.py:249-274) through scikit-learn itself: weighted f1 / recall / precision (zero_division=1) and the
weighted average precision of the binarised predictions at the thresholds 0.0 ... 0.5.

N = 83 rows x 15 classes of random probabilities and labels, no score within 1e-4 of a threshold, with a class without
support, a class never predicted (even at t = 0: its scores are 0), a class always predicted and rows without labels.
Stored: the inputs, the integer counts (TP / FP / FN per class per threshold, support) and the 24 scalars with their keys.

    python tools/gen_golden_ssl_online.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "ssl_online.npz")
SEED = 2025
THRESHOLDS = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)


def main() -> None:
    from tests import ssl_online_ref as R
    rng = np.random.default_rng(SEED)
    N, C = 83, 15
    y = (rng.random((N, C)) < 0.25).astype(np.uint8)
    p = rng.random((N, C)).astype(np.float32)
    for t in THRESHOLDS:
        p[np.abs(p - np.float32(t)) < 1e-4] += np.float32(1e-3)      # no score within rounding of a threshold
    y[:, 11] = 0                                     # a class without support
    p[:, 4] = 0.0                                    # a class never predicted, even at t = 0 (the comparison is strict)
    p[:, 7] = np.maximum(p[:, 7], 0.75)              # a class always predicted
    y[[2, 31, 60], :] = 0                            # rows without labels
    scalars = R.sklearn_scalars(p, y, THRESHOLDS)
    counts, support = R.sweep_counts(p, y, THRESHOLDS)
    keys = np.array(list(scalars))
    np.savez_compressed(OUT, probs=p, labels=y, thresholds=np.array(THRESHOLDS, dtype=np.float64), counts=counts,
                        support=support, keys=keys, scalars=np.array([scalars[k] for k in keys], dtype=np.float64))
    print(f"ssl_online: {OUT}; f1@0.3 {scalars['val/online/f1@0.3']:.6f}, avg_precision@0.3 "
          f"{scalars['val/online/avg_precision@0.3']:.6f}")


if __name__ == "__main__":
    main()
