"""The ranked metrics (ops.average_precision, ops.rank_metrics: one descending sort per class and the parallel rank pass
of csrc/eval_metrics.hip behind both) and the counts kernels against their bytes-moved floor, on the MI355X.

    python tools/bench_rank_metrics.py [--rounds 3] [--warmup 5] [--steps 30] [--sizes 653,6047,65536,1048576]
    python tools/bench_rank_metrics.py --one rank --n 65536        # one timing in this process (what the driver spawns)

Rows are [N, 19]: N = 653 and 6047 are the reference's validation and training splits (MMX_Light_dl.py:137-139).  The
driver runs ONE PROCESS PER TIMING, each under its own time limit, and takes the three calls in turn round by round on
the same GPU; a timing is hipEvents around one call after a warm-up, the median over the steps, and the driver reports
the median and the spread (min .. max) of the per-round medians.  One JSON line on stdout.

  ap            ops.average_precision: per-row AP and its mean, layout, segmented sort, aggregates, class pass, f32 outputs
  rank          ops.rank_metrics: layout, the same sort, aggregates, class pass, totals (AP + AUROC, macro / weighted)
  rank_all      the same with micro (a second, device-wide sort and pass over N C elements) and samples on
  confusion     ops.confusion_matrix from f32 logits [N, 305] (the MIT label set); floor = logits + targets read once
  confusion_i   ops.confusion_matrix from int64 predictions [N]
  ml_counts     ops.multilabel_counts [N, 19]; floor = probabilities + labels read once
  sklearn       roc_auc_score + average_precision_score(average=None) on the host, where scikit-learn is installed

The phases of a call (layout, sort, aggregates, class pass) are kernel times: run `--one rank --n N` under a kernel trace
(`rocprofv3 --kernel-trace --stats -- python ...`) in a run of its own; tracing slows the host, so the end-to-end numbers
come from the plain run."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C_ROWS = 19
C_MIT = 305
HBM_PEAK_GBS = 8000.0
CHILD_LIMIT_S = 240


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _time(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    q = lambda f: ms[min(len(ms) - 1, int(round(f * (len(ms) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2)}


def one(key: str, n: int, warmup: int, steps: int) -> dict:
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_metrics: no GPU visible; nothing is measured on a CPU")
    from dvt_amd import ops
    rng = np.random.default_rng(n)
    if key in ("ap", "rank", "rank_all", "ml_counts", "sklearn"):
        probs = rng.random((n, C_ROWS)).astype(np.float32)
        lab = (rng.random((n, C_ROWS)) < 0.3).astype(np.uint8)
        lab[0], lab[1] = 1, 0
        if key == "sklearn":
            from sklearn import metrics as M
            t0 = time.perf_counter()
            M.roc_auc_score(lab, probs, average=None)
            M.average_precision_score(lab, probs, average=None)
            return {"median_us": round((time.perf_counter() - t0) * 1e6, 1), "n_calls": 1}
        p, l = torch.from_numpy(probs).cuda(), torch.from_numpy(lab).cuda()
        if key == "ap":
            return _time(lambda: ops.average_precision(p, l), warmup, steps)
        if key == "rank":
            return _time(lambda: ops.rank_metrics(p, l), warmup, steps)
        if key == "rank_all":
            return _time(lambda: ops.rank_metrics(p, l, micro=True, samples=True), warmup, steps)
        state = ops.zeros((4, C_ROWS), torch.int64, p.device)
        r = _time(lambda: ops.multilabel_counts(p, l, 0.5, state), warmup, steps)
        r["floor_us"] = round(n * C_ROWS * 5 / (HBM_PEAK_GBS * 1e9) * 1e6, 2)
        return r
    target = torch.from_numpy(rng.integers(0, C_MIT, n).astype(np.int64)).cuda()
    cm, ign = ops.zeros((C_MIT, C_MIT), torch.int64, target.device), ops.zeros((1,), torch.int64, target.device)
    if key == "confusion":
        logits = torch.from_numpy(rng.standard_normal((n, C_MIT)).astype(np.float32)).cuda()
        r = _time(lambda: ops.confusion_matrix(logits, target, C_MIT, cm, ign), warmup, steps)
        r["floor_us"] = round(n * (C_MIT * 4 + 8) / (HBM_PEAK_GBS * 1e9) * 1e6, 2)
        return r
    if key == "confusion_i":
        pred = torch.from_numpy(rng.integers(0, C_MIT, n).astype(np.int64)).cuda()
        r = _time(lambda: ops.confusion_matrix(pred, target, C_MIT, cm, ign), warmup, steps)
        r["floor_us"] = round(n * 16 / (HBM_PEAK_GBS * 1e9) * 1e6, 2)
        return r
    raise SystemExit(f"unknown timing {key!r}")


def _child(key, n, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", key, "--n", str(n), "--warmup", str(a.warmup), "--steps",
           str(a.steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_rank_metrics: {key} at N = {n} ran past {CHILD_LIMIT_S} s; stopping")
    if r.returncode != 0:
        raise SystemExit(f"bench_rank_metrics: {key} at N = {n} failed ({r.returncode}); stopping\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default=None)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--sizes", default="653,6047,65536,1048576")
    ap.add_argument("--counts-n", type=int, default=262144)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.n, a.warmup, a.steps)))
        return
    res = {"classes": C_ROWS, "rounds": a.rounds, "warmup": a.warmup, "steps": a.steps, "rank": {}}
    for n in (int(s) for s in a.sizes.split(",")):
        per = {k: [] for k in ("ap", "rank", "rank_all")}
        for _ in range(a.rounds):                      # the calls take turns, a process each
            for k in per:
                per[k].append(_child(k, n, a)["median_us"])
        row = {k: {"median_us": round(_median(v), 2), "min_us": min(v), "max_us": max(v)} for k, v in per.items()}
        res["rank"][str(n)] = row
        print(f"[bench_rank_metrics] N = {n}: {row}", file=sys.stderr, flush=True)
    res["counts"] = {"n": a.counts_n}
    for k in ("confusion", "confusion_i", "ml_counts"):
        res["counts"][k] = _child(k, a.counts_n, a)
    try:
        import sklearn  # noqa: F401
        res["sklearn_host_65536"] = _child("sklearn", 65536, a)
    except ImportError:
        res["sklearn_host_65536"] = "not measured: scikit-learn is not installed"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
