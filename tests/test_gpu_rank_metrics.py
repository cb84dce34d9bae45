"""GPU checks of csrc/eval_metrics.hip through ops / metrics: the rank pass (AUROC, AP, averages) at sizes on the edges of
its block, the confusion-matrix and multilabel counts, and the torchmetrics-named objects, against the numpy restatement
(tests/rank_metrics_ref.py) and the scikit-learn fixture (tests/golden/rank_metrics.npz); never against scikit-learn itself.

Integers must match exactly.  Floats: 1e-12 absolute -- both sides are float64 ratios of integers < 2^53, and AP / the
averages are sums of at most a few thousand such terms in [0, 1] taken in different orders (<= 6144 * 2^-53 = 7e-13)."""
import os

import numpy as np
import pytest
import torch

from tests import rank_metrics_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_metrics.npz")
TOL = 1e-12
KINDS = ("cont", "q1", "q2", "q8", "ascending", "zeros", "bf16")
CLASSES = (1, 19, 64)


def _block():
    from dvt_amd import ops
    return ops.rank_metrics_block()


def _sizes():
    bk = 2048            # dvt_rank_metrics_block(); test_sizes_sit_on_the_block_edges pins the two together
    return (1, 2, 255, 256, 257, bk - 1, bk, bk + 1, 2 * bk + 1, 3 * bk)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def make_labels(rng, N, C):
    lab = (rng.random((N, C)) < 0.3).astype(np.uint8)
    if N >= 2:
        lab[0], lab[1] = 1, 0
    return lab


def make_scores(rng, N, C, kind):
    """-> (scores as handed to the device: a float32 array, or a bfloat16 tensor; the float32 values they stand for)."""
    x = rng.random((N, C)).astype(np.float32)
    if kind in ("q1", "q2", "q8"):
        q = int(kind[1:])
        x = (np.floor(x * q) / q).astype(np.float32)          # q1: one tie group across every block
    elif kind == "ascending":
        x = np.sort(x, axis=0)                                 # already sorted the wrong way round
    elif kind == "zeros":
        pick = rng.integers(0, 3, N)
        x[:, 0] = np.where(pick == 0, np.float32(-0.0), np.where(pick == 1, np.float32(0.0), np.float32(0.5)))
    elif kind == "bf16":
        t = torch.from_numpy(x).to(torch.bfloat16)
        return t, t.float().numpy()
    return x, x


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(want)).max() if got.size else 0.0
    assert d <= TOL, d


def check_rank(r, ref, micro=True, samples=True):
    assert np.array_equal(r.two_u.cpu().numpy(), ref["two_u"])
    assert np.array_equal(r.positives.cpu().numpy(), ref["positives"])
    close(r.auroc.cpu().numpy(), ref["auroc"])
    close(r.ap.cpu().numpy(), ref["ap"])
    close(r.macro.item(), ref["macro"])
    close(r.weighted.item(), ref["weighted"])
    assert int(r.valid_classes) == ref["valid_classes"]
    if micro:
        assert (int(r.micro_two_u), int(r.micro_positives)) == (ref["micro_two_u"], ref["micro_positives"])
        close(r.micro.item(), ref["micro"])
    if samples:
        assert int(r.valid_rows) == ref["valid_rows"]
        close(r.samples_sum.item(), ref["samples_sum"])


def test_sizes_sit_on_the_block_edges():
    assert _block() == 2048 and _sizes()[5:8] == (_block() - 1, _block(), _block() + 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", _sizes())
def test_rank_pass_against_the_oracle(device, N, kind):
    from dvt_amd import ops
    for C in CLASSES:
        rng = np.random.default_rng([N, C, KINDS.index(kind)])
        scores, values = make_scores(rng, N, C, kind)
        lab = make_labels(rng, N, C)
        dev = (scores if torch.is_tensor(scores) else torch.from_numpy(scores)).to(device)
        r = ops.rank_metrics(dev, torch.from_numpy(lab).to(device), micro=True, samples=True)
        check_rank(r, R.rank_metrics(values, lab))


def test_rank_pass_on_the_fixture(device, gold):
    from dvt_amd import ops
    for case in ("cont_1025x19", "q2_255x19", "q8_257x19", "q16_300x15", "equalcol_257x6"):
        probs, lab = gold[f"{case}/probs"], gold[f"{case}/labels"]
        r = ops.rank_metrics(torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device), micro=True, samples=True)
        close(r.auroc.cpu().numpy(), gold[f"{case}/auroc"])
        close(r.ap.cpu().numpy(), gold[f"{case}/ap"])
        close(r.macro.item(), gold[f"{case}/auroc_macro"])
        close(r.weighted.item(), gold[f"{case}/auroc_weighted"])
        close(r.micro.item(), gold[f"{case}/auroc_micro"])
        assert int(r.valid_rows) == int(gold[f"{case}/valid_rows"])
        close(r.samples_sum.item() / int(r.valid_rows), gold[f"{case}/auroc_samples"])


def test_degenerate_classes_are_nan_and_left_out(device):
    from dvt_amd import ops
    N, C = 257, 19
    rng = np.random.default_rng(257)
    probs, lab = rng.random((N, C)).astype(np.float32), make_labels(rng, N, C)
    lab[:, 3], lab[:, 11] = 1, 0                              # one class all positive, one all negative
    r = ops.rank_metrics(torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device), micro=True, samples=True)
    ref = R.rank_metrics(probs, lab)
    check_rank(r, ref)
    a, ap = r.auroc.cpu().numpy(), r.ap.cpu().numpy()
    assert np.array_equal(np.nonzero(np.isnan(a))[0], [3, 11])
    assert int(r.valid_classes) == C - 2 == ref["valid_classes"]
    assert ap[11] == 0.0 and abs(ap[3] - 1.0) <= TOL         # no positives: 0; all positive: precision 1 at every cut
    assert not np.isnan(r.macro.item()) and not np.isnan(r.weighted.item())
    # without the flags the optional outputs say so
    r = ops.rank_metrics(torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device))
    assert np.isnan(r.micro.item()) and np.isnan(r.samples_sum.item())
    assert (int(r.valid_rows), int(r.micro_two_u), int(r.micro_positives)) == (-1, -1, -1)
    check_rank(r, ref, micro=False, samples=False)


def test_more_than_64_classes_without_the_per_row_part(device):
    from dvt_amd import ops
    N, C = 300, 80
    rng = np.random.default_rng(80)
    probs, lab = make_scores(rng, N, C, "q8")[1], make_labels(rng, N, C)
    p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
    check_rank(ops.rank_metrics(p, l, micro=True), R.rank_metrics(probs, lab, samples=False), samples=False)
    with pytest.raises(RuntimeError, match="64 classes"):
        ops.rank_metrics(p, l, samples=True)


def test_repeated_call_is_bitwise_equal_and_average_precision_is_unchanged(device):
    from dvt_amd import ops
    bk = _block()
    N, C = 2 * bk + 1, 19
    rng = np.random.default_rng(7)
    probs, lab = make_scores(rng, N, C, "q8")[1], make_labels(rng, N, C)
    p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
    a = ops.rank_metrics(p, l, micro=True, samples=True)
    a = [t.clone() for t in a]
    b = ops.rank_metrics(p, l, micro=True, samples=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)
    # the existing AP entry point (f32 outputs) on the same inputs: same values, and the same from call to call
    _, w1, per1 = (t.clone() for t in ops.average_precision(p, l))
    _, w2, per2 = ops.average_precision(p, l)
    assert torch.equal(per1, per2) and torch.equal(w1, w2)
    assert np.abs(per1.cpu().numpy().astype(np.float64) - b.ap.cpu().numpy()).max() <= 1e-6


@pytest.mark.parametrize("N", (1, 2, 257, 2049))
def test_average_precision_is_the_rank_pass_rounded_to_f32(device, N):
    """ops.average_precision takes its per-class values from the rank pass: the f64 AP of ops.rank_metrics rounded to f32,
    bit for bit, and the weighted value formed from those f32 values and the integer supports in class order."""
    from dvt_amd import ops
    assert 2049 == _block() + 1
    for C in CLASSES:
        for blank in sorted({C // 2, C - 1}) + ([None] if C == 1 else []):     # a class without positives (C = 1: also with)
            rng = np.random.default_rng([N, C, 8])
            probs, lab = make_scores(rng, N, C, "q8")[1], make_labels(rng, N, C)
            if blank is not None:
                lab[:, blank] = 0
            p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
            _, w1, per1 = (t.clone() for t in ops.average_precision(p, l))
            _, w2, per2 = ops.average_precision(p, l)
            assert torch.equal(per1.view(torch.int32), per2.view(torch.int32))
            assert torch.equal(w1.view(torch.int32), w2.view(torch.int32))
            r = ops.rank_metrics(p, l)
            assert torch.equal(per1.view(torch.int32), r.ap.float().view(torch.int32)), (N, C, blank)
            ap32, pos = per1.cpu().numpy(), r.positives.cpu().numpy()
            assert np.array_equal(pos, lab.sum(0)) and (blank is None or (pos[blank] == 0 and ap32[blank] == 0.0))
            num = den = 0.0
            for c in range(C):                                                  # the kernel's order: class by class, in f64
                num += float(ap32[c]) * float(pos[c])
                den += float(pos[c])
            want = np.float32(num / den) if den > 0 else np.float32(0.0)
            assert w1.cpu().numpy()[0].tobytes() == want.tobytes(), (N, C, blank, w1, want)


@pytest.mark.parametrize("N", (1, 255, 257, 4097))
def test_report_counts_are_the_sweep_counts_at_one_threshold(device, N):
    from dvt_amd import ops
    th = 0.5
    for C in (1, 19):
        rng = np.random.default_rng([N, C, 5])
        probs, lab = rng.random((N, C)).astype(np.float32), make_labels(rng, N, C)
        probs[::3, 0] = th                                    # equal to the threshold: strict > leaves them negative
        p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
        counts, _ = ops.multilabel_report_counts(p, l, th)
        sweep, support = ops.multilabel_sweep_counts(p, l, [th])
        assert counts.dtype == sweep.dtype == support.dtype == torch.int64
        assert torch.equal(counts[:3], sweep[0]) and torch.equal(counts[3], support)
        pred, truth = probs > np.float32(th), lab != 0
        want = np.stack([(pred & truth).sum(0), (pred & ~truth).sum(0), (~pred & truth).sum(0), truth.sum(0)])
        assert not pred[::3, 0].any() and np.array_equal(counts.cpu().numpy(), want)


def test_f1_samples_and_average_precision_refuse_mismatched_shapes(device):
    from dvt_amd import ops
    p = torch.zeros((8, 19), dtype=torch.float32, device=device)
    for bad in (torch.zeros((8, 18), dtype=torch.uint8, device=device), torch.zeros((7, 19), dtype=torch.uint8, device=device),
                torch.zeros((8 * 19,), dtype=torch.uint8, device=device)):
        with pytest.raises(ValueError, match="f1_samples"):
            ops.f1_samples(p, bad, (0.5,))
        with pytest.raises(ValueError, match="average_precision"):
            ops.average_precision(p, bad)


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("C", (2, 22, 305))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 4097))
def test_confusion_matrix_counts(device, N, C):
    from dvt_amd import ops
    rng = np.random.default_rng([N, C])
    logits = rng.standard_normal((N, C)).astype(np.float32)
    target = rng.integers(0, C, N).astype(np.int64)
    logits[0] = 0.25                                          # every class ties: index 0
    if N > 5:
        logits[5, C // 2:] = 9.0                              # a tie that starts away from index 0
    want_pred = R.argmax_lowest(logits)
    assert want_pred[0] == 0 and (N <= 5 or want_pred[5] == C // 2)
    want, _ = R.confusion_matrix(want_pred, target, C)
    t = torch.from_numpy(target).to(device)
    cm, ign = ops.confusion_matrix(torch.from_numpy(logits).to(device), t, C)
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), want) and int(ign) == 0
    cm, ign = ops.confusion_matrix(torch.from_numpy(want_pred).to(device), t, C)
    assert np.array_equal(cm.cpu().numpy(), want) and int(ign) == 0
    # bf16 logits: the argmax of the rounded values (rounding makes more ties; the lowest index still wins)
    lb = torch.from_numpy(logits).to(torch.bfloat16)
    want_b, _ = R.confusion_matrix(R.argmax_lowest(lb.float().numpy()), target, C)
    cm_b, _ = ops.confusion_matrix(lb.to(device), t, C)
    assert np.array_equal(cm_b.cpu().numpy(), want_b)
    # targets outside [0, C) are skipped and counted; accumulating the same batch again doubles everything
    bad = target.copy()
    bad[::7] = np.where(np.arange(len(bad[::7])) % 2 == 0, -1, C)
    want2, skipped = R.confusion_matrix(want_pred, bad, C)
    cm2, ign2 = ops.confusion_matrix(torch.from_numpy(logits).to(device), torch.from_numpy(bad).to(device), C)
    assert np.array_equal(cm2.cpu().numpy(), want2) and int(ign2) == skipped == len(bad[::7])
    ops.confusion_matrix(torch.from_numpy(logits).to(device), torch.from_numpy(bad).to(device), C, cm2, ign2)
    assert np.array_equal(cm2.cpu().numpy(), 2 * want2) and int(ign2) == 2 * skipped


@pytest.mark.parametrize("C", (1, 15, 19, 64))
def test_multilabel_counts(device, C):
    from dvt_amd import ops
    N, th = 1531, 0.5
    rng = np.random.default_rng(C)
    probs, lab = rng.random((N, C)).astype(np.float32), make_labels(rng, N, C)
    probs[::5, 0] = th                                        # equal to the threshold: strict > leaves them negative
    want = R.multilabel_counts(probs, lab, th)
    assert want[0, 0] + want[1, 0] <= N - len(probs[::5])
    p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
    one = ops.multilabel_counts(p, l, th)
    assert one.dtype == torch.int64 and np.array_equal(one.cpu().numpy(), want)
    assert torch.equal(ops.multilabel_counts(p, l, th), one)
    state = ops.zeros((4, C), torch.int64, device)
    for lo, hi in ((0, 1), (1, 700), (700, N)):               # three uneven batches
        ops.multilabel_counts(p[lo:hi], l[lo:hi], th, state)
    assert torch.equal(state, one)
    # the sweep kernel's comparison: TP / FP / FN agree with it at the same threshold
    counts, _ = ops.multilabel_sweep_counts(p, l, (th,))
    assert torch.equal(counts[0], one[:3])


BATCHES = ((0, 0.1), (0.1, 0.55), (0.55, 1.0))                # three uneven batches, as fractions of the rows


def _batches(n):
    return [(int(a * n), int(b * n)) for a, b in BATCHES]


@pytest.mark.parametrize("case", ("mc_301x22", "mc_65x2", "mc_120x305"))
def test_f1_and_confusion_matrix_multiclass_on_the_fixture(device, gold, case):
    from dvt_amd import metrics
    logits = torch.from_numpy(gold[f"{case}/logits"]).to(device)
    target = torch.from_numpy(gold[f"{case}/target"]).to(device)
    Cn = logits.shape[1]
    cmo = metrics.ConfusionMatrix(Cn)
    objs = {avg: metrics.F1(Cn, average=avg) for avg in ("micro", "macro", "weighted", "none")}
    for lo, hi in _batches(logits.shape[0]):
        cmo(logits[lo:hi], target[lo:hi])
        for o in objs.values():
            o(logits[lo:hi], target[lo:hi])
    cm = cmo.compute()
    assert cm.is_cuda and cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), gold[f"{case}/cm"])
    assert int(cmo.ignored) == 0
    for avg, o in objs.items():
        got = o.compute()
        assert got.dtype == torch.float64
        assert np.abs(got.numpy() - gold[f"{case}/f1_{avg}"]).max() <= TOL, avg
    # the functionals in one shot, from integer predictions
    pred = torch.from_numpy(gold[f"{case}/pred"]).to(device)
    assert torch.equal(metrics.confusion_matrix(pred, target, Cn), cm)
    assert abs(float(metrics.f1(pred, target, Cn, average="macro")) - float(gold[f"{case}/f1_macro"])) <= TOL
    objs["micro"].reset()
    with pytest.raises(RuntimeError, match="before any update"):
        objs["micro"].compute()


@pytest.mark.parametrize("case", ("ml_653x19", "ml_97x15", "ml_33x1"))
def test_f1_and_confusion_matrix_multilabel_on_the_fixture(device, gold, case):
    from dvt_amd import metrics
    probs = torch.from_numpy(gold[f"{case}/probs"]).to(device)
    lab = torch.from_numpy(gold[f"{case}/labels"]).to(device)
    Cn, th = probs.shape[1], float(gold["threshold"])
    averages = ("micro", "macro", "weighted", "none") + (("samples",) if Cn > 1 else ())
    cmo = metrics.ConfusionMatrix(Cn, multilabel=True, threshold=th)
    objs = {avg: metrics.F1(Cn, threshold=th, average=avg) for avg in averages}
    for lo, hi in _batches(probs.shape[0]):
        cmo(probs[lo:hi], lab[lo:hi])
        for o in objs.values():
            o(probs[lo:hi], lab[lo:hi])
    mcm = cmo.compute()
    assert tuple(mcm.shape) == (Cn, 2, 2) and np.array_equal(mcm.cpu().numpy(), gold[f"{case}/mcm"])
    for avg, o in objs.items():
        assert np.abs(o.compute().numpy() - gold[f"{case}/f1_{avg}"]).max() <= TOL, avg
    assert torch.equal(metrics.confusion_matrix(probs, lab, Cn, multilabel=True, threshold=th), mcm)
    with pytest.raises(ValueError, match="multilabel"):
        metrics.F1(Cn, average="samples").update((probs[:, 0] > th).long(), lab[:, 0].long())


class _Module:
    def __init__(self):
        self.running_logits, self.running_labels, self.logged = [], [], {}

    def log(self, name, value, **kw):
        self.logged[name] = value


def test_mit_eval_logs_the_accuracy_and_resets(device, gold):
    from dvt_amd import metrics
    case = "mc_301x22"
    pred = torch.from_numpy(gold[f"{case}/pred"]).to(device)
    target = torch.from_numpy(gold[f"{case}/target"]).to(device)
    m = _Module()
    for lo, hi in _batches(pred.shape[0]):
        m.running_logits.append(pred[lo:hi])
        m.running_labels.append(target[lo:hi])
    cb = metrics.MITEval()
    acc = cb.on_validation_epoch_end(None, m)
    assert abs(acc - float(gold[f"{case}/accuracy"])) <= TOL and m.logged == {"val/accuracy/epoch": acc}
    assert m.running_logits == [] and m.running_labels == [] and cb.best_acc == 0


def test_count_equal(device):
    from dvt_amd import ops
    rng = np.random.default_rng(3)
    for n in (1, 255, 4097, 70001):
        a, b = rng.integers(0, 3, n), rng.integers(0, 3, n)
        ta, tb = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
        out = ops.count_equal(ta, tb)
        assert out.dtype == torch.int64 and int(out) == int((a == b).sum())
        ops.count_equal(ta.float(), tb.float(), out)
        assert int(out) == 2 * int((a == b).sum())


def test_auroc_streamed_equals_one_shot(device):
    """A FrameTransformer-shaped stream of [2, 19] batches for 40 steps."""
    from dvt_amd import metrics
    rng = np.random.default_rng(40)
    probs, lab = rng.random((80, 19)).astype(np.float32), make_labels(rng, 80, 19)
    p, l = torch.from_numpy(probs).to(device), torch.from_numpy(lab).to(device)
    ref = R.rank_metrics(probs, lab)
    want = {"macro": ref["macro"], "weighted": ref["weighted"], "micro": ref["micro"],
            "samples": ref["samples_sum"] / ref["valid_rows"], "none": ref["auroc"]}
    for avg in ("macro", "weighted", "micro", "samples", "none"):
        m = metrics.AUROC(19, average=avg)
        for i in range(40):
            m(p[2 * i:2 * i + 2], l[2 * i:2 * i + 2].float())
        got = m.compute()
        assert got.is_cuda and got.dtype == torch.float64
        one = metrics.auroc(p, l, average=avg)
        assert torch.equal(got, one)
        close(got.cpu().numpy(), want[avg])
        m.reset()
        with pytest.raises(RuntimeError, match="before any update"):
            m.compute()
