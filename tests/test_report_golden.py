"""The test epoch's classification_report (callbacks.py:67-82): the numpy restatement against scikit-learn's own values
(tests/golden/test_report.npz, written by tools/gen_golden_report.py), and the package's report assembly from counts."""
import numpy as np
import torch

from tests import report_ref as R
from tests.util import golden


def test_restatement_matches_sklearn_fixture():
    g = golden("test_report.npz")
    t = float(g["threshold"])
    per_class, averages = R.report_arrays(g["probs"], g["labels"], t)
    assert np.array_equal(R.counts(g["probs"], g["labels"], t), g["counts"])
    assert np.abs(per_class - g["per_class"]).max() < 1e-12
    assert np.abs(averages - g["averages"]).max() < 1e-12
    assert g["counts"][3, 14] == 0 and g["counts"][0, 5] + g["counts"][1, 5] == 0      # no support / never predicted
    assert (g["labels"].sum(1) == 0).sum() >= 3


def test_report_from_counts_matches_sklearn_fixture():
    from dvt_amd.metrics import format_report, report_from_counts
    g = golden("test_report.npz")
    t = float(g["threshold"])
    p, y = g["probs"], g["labels"]
    pr, yy = (p > np.float32(t)).astype(np.int64), y.astype(np.int64)
    rtp, rp, rt = (pr & yy).sum(1), pr.sum(1), yy.sum(1)
    sums = [R._div(rtp, rp).sum(), R._div(rtp, rt).sum(), R._div(2 * rtp, rp + rt).sum()]
    names = [f"c{i}" for i in range(19)]
    rep = report_from_counts(torch.from_numpy(g["counts"]), torch.tensor(sums, dtype=torch.float64), p.shape[0], names)
    assert list(rep) == names + list(R.AVERAGES)
    for i, n in enumerate(names):
        assert list(rep[n]) == list(R.FIELDS)
        assert np.abs(np.array([rep[n][f] for f in R.FIELDS]) - g["per_class"][i]).max() < 1e-12
    for i, a in enumerate(R.AVERAGES):
        assert np.abs(np.array([rep[a][f] for f in R.FIELDS]) - g["averages"][i]).max() < 1e-12
    text = format_report(rep)
    assert "samples avg" in text and text.count("\n") == len(rep) + 3
