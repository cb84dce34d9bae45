"""CPU-side checks of the rank metrics and counts: the numpy restatement (tests/rank_metrics_ref.py) against the scikit-learn
fixture (tests/golden/rank_metrics.npz, tools/gen_golden_rank_metrics.py), the public names and their refusals, the
declarations in the header and the binding, ``metrics.f1_from_counts`` on the fixture's counts, and ``metrics.reduce_counts``
over gloo with two processes."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import rank_metrics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_metrics.npz")
TOL = 1e-12          # both sides are float64 ratios of integers < 2^53 and sums of at most a few thousand terms
RANK_CASES = ("cont_1025x19", "cont_64x1", "q1_130x5", "q2_255x19", "q4_257x7", "q8_257x19", "q16_300x15", "equalcol_257x6")
MULTICLASS_CASES = ("mc_301x22", "mc_65x2", "mc_120x305")
MULTILABEL_CASES = ("ml_653x19", "ml_97x15", "ml_33x1")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("case", RANK_CASES)
def test_oracle_matches_scikit_learn_rank(gold, case):
    probs, lab = gold[f"{case}/probs"], gold[f"{case}/labels"]
    r = R.rank_metrics(probs, lab)
    assert r["two_u"].dtype == np.int64 and np.array_equal(r["positives"], lab.astype(np.int64).sum(0))
    assert np.abs(r["auroc"] - gold[f"{case}/auroc"]).max() <= TOL
    assert np.abs(r["ap"] - gold[f"{case}/ap"]).max() <= TOL
    if probs.shape[1] > 1:
        assert abs(r["macro"] - gold[f"{case}/auroc_macro"]) <= TOL
        assert abs(r["weighted"] - gold[f"{case}/auroc_weighted"]) <= TOL
        assert abs(r["micro"] - gold[f"{case}/auroc_micro"]) <= TOL
        assert r["valid_rows"] == int(gold[f"{case}/valid_rows"])
        assert abs(r["samples_sum"] / r["valid_rows"] - gold[f"{case}/auroc_samples"]) <= TOL
        w = r["positives"] / r["positives"].sum()
        assert abs(float(np.mean(r["ap"])) - gold[f"{case}/ap_macro"]) <= TOL
        assert abs(float(np.sum(r["ap"] * w)) - gold[f"{case}/ap_weighted"]) <= TOL
        assert abs(R.column(probs.reshape(-1), lab.reshape(-1))[3] - gold[f"{case}/ap_micro"]) <= TOL


def test_oracle_degenerate_columns_and_signed_zeros():
    s = np.array([0.5, 0.25, 0.75], dtype=np.float32)
    u, p, a, ap = R.column(s, [1, 1, 1])
    assert (u, p, ap) == (0, 3, 1.0) and np.isnan(a)
    u, p, a, ap = R.column(s, [0, 0, 0])
    assert (p, ap) == (0, 0.0) and np.isnan(a)
    # -0.0 and +0.0 tie: one positive and one negative in one group -> AUROC 0.5
    u, p, a, ap = R.column(np.array([-0.0, 0.0], dtype=np.float32), [1, 0])
    assert (u, p, a, ap) == (1, 1, 0.5, 0.5)
    # hand-worked: scores 3 2 2 1, labels 1 0 1 0 -> groups {1+}, {1+, 1-}, {1-}: 2U = 1*(2*1 + 1) + 1*(2*2 + 0) = 7
    u, p, a, ap = R.column(np.array([3, 2, 2, 1], dtype=np.float32), [1, 0, 1, 0])
    assert (u, p) == (7, 2) and a == 7 / 8 and abs(ap - (0.5 * 1.0 + 0.5 * (2 / 3))) <= 1e-16


@pytest.mark.parametrize("case", MULTICLASS_CASES)
def test_oracle_matches_scikit_learn_multiclass(gold, case):
    logits, target = gold[f"{case}/logits"], gold[f"{case}/target"]
    Cn = logits.shape[1]
    pred = R.argmax_lowest(logits)
    assert np.array_equal(pred, gold[f"{case}/pred"]) and pred[3] == 0
    cm, skipped = R.confusion_matrix(pred, target, Cn)
    assert skipped == 0 and np.array_equal(cm, gold[f"{case}/cm"])
    tp = np.diag(cm)
    fp, fn = cm.sum(0) - tp, cm.sum(1) - tp
    for avg in ("micro", "macro", "weighted", "none"):
        assert np.abs(R.f1_from_counts(tp, fp, fn, avg) - gold[f"{case}/f1_{avg}"]).max() <= TOL, avg
    assert abs(R.accuracy(pred, target) - gold[f"{case}/accuracy"]) <= TOL
    bad = target.copy()
    bad[:2] = (-1, Cn)
    cm2, skipped = R.confusion_matrix(pred, bad, Cn)
    assert skipped == 2 and cm2.sum() == len(target) - 2


@pytest.mark.parametrize("case", MULTILABEL_CASES)
def test_oracle_matches_scikit_learn_multilabel(gold, case):
    probs, lab, th = gold[f"{case}/probs"], gold[f"{case}/labels"], float(gold["threshold"])
    counts = R.multilabel_counts(probs, lab, th)
    assert np.array_equal(counts.sum(0), np.full(probs.shape[1], probs.shape[0]))
    assert np.array_equal(R.multilabel_confusion(counts), gold[f"{case}/mcm"])
    for avg in ("micro", "macro", "weighted", "none"):
        assert np.abs(R.f1_from_counts(counts[0], counts[1], counts[2], avg) - gold[f"{case}/f1_{avg}"]).max() <= TOL, avg
    if probs.shape[1] > 1:
        assert abs(R.f1_samples(probs > np.float32(th), lab) - gold[f"{case}/f1_samples"]) <= TOL


@pytest.mark.parametrize("case", MULTICLASS_CASES + MULTILABEL_CASES)
def test_f1_from_counts_on_the_host(gold, case):
    """metrics.f1_from_counts, the float64 ratios F1.compute() forms from the integer state."""
    from dvt_amd import metrics
    if case in MULTICLASS_CASES:
        cm = gold[f"{case}/cm"]
        tp = np.diag(cm)
        fp, fn = cm.sum(0) - tp, cm.sum(1) - tp
    else:
        tp, fp, fn, _ = R.multilabel_counts(gold[f"{case}/probs"], gold[f"{case}/labels"], float(gold["threshold"]))
    for avg in ("micro", "macro", "weighted", "none"):
        got = metrics.f1_from_counts(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (tp, fp, fn)), avg)
        assert got.dtype == torch.float64
        assert np.abs(got.numpy() - gold[f"{case}/f1_{avg}"]).max() <= TOL, avg


def test_public_names_and_refusals():
    from dvt_amd import metrics, ops
    for name in ("AUROC", "F1", "ConfusionMatrix", "MITEval", "auroc", "f1", "confusion_matrix", "reduce_counts"):
        assert hasattr(metrics, name), name
    for name in ("rank_metrics", "confusion_matrix", "multilabel_counts", "count_equal", "rank_metrics_block"):
        assert callable(getattr(ops, name)), name
    assert metrics.AUROC(19).average == "macro" and metrics.AUROC(19, average=None).average == "none"
    assert metrics.F1(22).average == "micro" and metrics.F1(22).threshold == 0.5
    assert metrics.ConfusionMatrix(305).multilabel is False and metrics.MITEval().best_acc == 0
    for cls in (metrics.AUROC, metrics.F1):
        with pytest.raises(ValueError, match="average"):
            cls(19, average="median")
    for cls in (metrics.AUROC, metrics.F1, metrics.ConfusionMatrix):
        for bad in (0, -3, 2.5, None):
            with pytest.raises(ValueError, match="num_classes"):
                cls(bad)
        with pytest.raises(RuntimeError, match="before any update"):
            cls(19).compute()
    with pytest.raises(ValueError, match="19 classes"):
        metrics.AUROC(19).update(torch.zeros(4, 15), torch.zeros(4, 15))
    with pytest.raises(ValueError):                                   # wrong class count, multilabel and multiclass
        metrics.F1(19).update(torch.zeros(4, 15), torch.zeros(4, 15))
    with pytest.raises(ValueError):
        metrics.F1(19).update(torch.zeros(4, 15), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="multilabel"):
        metrics.ConfusionMatrix(19, multilabel=True).update(torch.zeros(4, 19), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):                    # no CPU path behind the wrappers
        ops.rank_metrics(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.multilabel_counts(torch.zeros(4, 3), torch.zeros(4, 3), 0.5)


def test_reduce_counts_without_a_process_group_is_the_identity():
    from dvt_amd import metrics
    s = torch.arange(12, dtype=torch.int64).view(4, 3)
    assert metrics.reduce_counts(s) is s


def test_header_declares_the_entry_points():
    from dvt_amd import _lib
    S = _lib.SIGNATURES
    assert S["dvt_rank_metrics_block"] == (C.c_int, [])
    assert S["dvt_rank_metrics_workspace_bytes"] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int])
    res, args = S["dvt_rank_metrics"]
    assert res is C.c_int and len(args) == 13 and args[2:5] == [C.c_int64, C.c_int, C.c_int]
    assert all(a is C.c_void_p for a in args[:2] + args[5:])
    assert len(S["dvt_confusion_matrix"][1]) == 10 and len(S["dvt_multilabel_counts"][1]) == 8
    assert S["dvt_multilabel_counts"][1][4] is C.c_float and len(S["dvt_count_equal"][1]) == 7
    assert _lib.ENUMS["dvt_rank_flags"] == {"DVT_RANK_MICRO": 1, "DVT_RANK_SAMPLES": 2}
    assert sorted(_lib.ENUMS["dvt_rank_average"].values()) == list(range(_lib.MACROS["DVT_RANK_N_AVERAGES"]))
    assert sorted(_lib.ENUMS["dvt_rank_count"].values()) == list(range(_lib.MACROS["DVT_RANK_N_COUNTS"]))
    assert _lib.ABI_VERSION == 5


def test_library_exports_and_validates_before_touching_the_gpu():
    from dvt_amd import _lib
    lib = _lib.load()
    bk = lib.dvt_rank_metrics_block()
    assert bk >= 256 and bk % 64 == 0
    assert lib.dvt_rank_metrics_workspace_bytes(0, 19, 0) == 0 and lib.dvt_rank_metrics_workspace_bytes(1 << 27, 19, 0) == 0
    assert lib.dvt_rank_metrics(None, None, 4, 3, 0, None, None, None, None, None, None, None, None) != 0
    assert b"dvt_rank_metrics" in lib.dvt_last_error()
    assert lib.dvt_confusion_matrix(None, _lib.F32, None, None, 4, 3, 0, None, None, None) != 0
    assert lib.dvt_multilabel_counts(None, None, 4, 3, 0.5, 0, None, None) != 0
    assert lib.dvt_count_equal(None, None, 4, 1, 0, None, None) != 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _split_state(rank):
    """Rank 0 holds the first 20 rows of the multilabel case, rank 1 the rest: [4, C] counts and a [C, C] matrix."""
    g = dict(np.load(GOLDEN))
    probs, lab = g["ml_97x15/probs"], g["ml_97x15/labels"]
    rows = slice(0, 20) if rank == 0 else slice(20, None)
    counts = R.multilabel_counts(probs[rows], lab[rows], float(g["threshold"]))
    pred, target = g["mc_301x22/pred"], g["mc_301x22/target"]
    rows = slice(0, 100) if rank == 0 else slice(100, None)
    cm, _ = R.confusion_matrix(pred[rows], target[rows], 22)
    return torch.from_numpy(counts), torch.from_numpy(cm)


def _reduce_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dvt_amd.metrics import reduce_counts
    counts, cm = _split_state(rank)
    keep = counts.clone()
    total, total_cm = reduce_counts(counts), reduce_counts(cm)
    assert torch.equal(counts, keep) and total.dtype == torch.int64          # the rank's own state is left as it is
    if rank == 0:
        out.put((total.numpy(), total_cm.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_counts_over_two_ranks_equals_the_concatenated_data():
    import dvt_amd  # noqa: F401  (registers the package alias before spawn pickles the worker)
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    total, total_cm = out.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    g = dict(np.load(GOLDEN))
    want = R.multilabel_counts(g["ml_97x15/probs"], g["ml_97x15/labels"], float(g["threshold"]))
    assert np.array_equal(total, want)
    assert np.array_equal(total_cm, g["mc_301x22/cm"])
