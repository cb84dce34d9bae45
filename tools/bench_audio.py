"""The VGGish audio expert at 256 one-second chunks (8 clips x 32) on the MI355X, timed with hipEvents (warm-up, then the
median over the timed iterations).  One JSON line on stdout.

    timeout -k 10 600 python tools/bench_audio.py [--warmup 5] [--steps 30] [--chunks 256]

Per compute dtype (bf16, fp32):
  front_end_fft / front_end_dft   dvt_logmel_examples with each form of the spectrum, ALTERNATED in one timed loop (the kept
                 form is ops.LOGMEL_VARIANT), and each form's max-abs error against the float64 restatement on eight chunks
  conv1_pool     dvt_vggish_conv1_pool
  conv_<i> / pool_<i> / fc_<i>    every remaining layer on its own input
  expert         VGGish.forward, waveform to embeddings
  eager_stack / eager_<layer>     torch's own eager modules (the VGG stack of tests/audio_ref.py, NCHW) on the same GPU and
                 the same examples, in the same dtype
The GEMM route of the three Linears at M = 1, 32 and the bench's M is recorded (ops.gemm_is_launch_bound, ops.gemm_plan).
Every figure is a time of this process's own launches; nothing is a share of peak.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2), "n": len(s)}


def _time(fns, warmup, steps):
    """Time the callables of ``fns`` alternately -> one list of milliseconds per callable."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(steps)]
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[row[i][0].elapsed_time(row[i][1]) for row in ev] for i in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--chunks", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio needs the MI355X: a timing on the CPU says nothing")
    from dvt_amd import _lib as L, ops
    from dvt_amd.models.pretrained import vggish
    from dvt_amd.models.pretrained.vggish import _CONVS, _K3, _P1, _S1
    from tests import audio_ref as A

    n = a.chunks
    wave_np = np.stack([A.seeded_waveform(s) for s in range(n)])
    wave = torch.from_numpy(wave_np).cuda()
    res = {"chunks": n, "warmup": a.warmup, "steps": a.steps, "kept_variant": ops.LOGMEL_VARIANT}
    r64 = A.logmel_examples(wave_np[:8])
    res["front_end_error_fp32_chain"] = float(np.abs(A.logmel_examples(wave_np[:8], np.float32) - r64).max())
    for v in ("fft", "dft"):
        got = ops.logmel_examples(wave[:8], torch.float32, v).cpu().numpy().astype(np.float64)
        res[f"front_end_error_{v}"] = float(np.abs(got - r64).max())

    net = vggish(compute_dtype=torch.float32).cuda()
    for mode, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        out = res[mode] = {}
        net.compute_dtype = dt
        t_fft, t_dft = _time([lambda: ops.logmel_examples(wave, dt, "fft"), lambda: ops.logmel_examples(wave, dt, "dft")],
                             a.warmup, a.steps)
        out["front_end_fft"], out["front_end_dft"] = _stats(t_fft), _stats(t_dft)
        ex = ops.logmel_examples(wave, dt)
        pk = net._packed(wave.device)
        with torch.no_grad():
            out["conv1_pool"] = _stats(_time([lambda: ops.vggish_conv1_pool(ex, *pk["conv1"])], a.warmup, a.steps)[0])
            y = ops.vggish_conv1_pool(ex, *pk["conv1"])
            for (idx, _cin, cout, H, W, pool), (w, b) in zip(_CONVS, pk["convs"]):
                f = lambda y=y, w=w, b=b, H=H, W=W, cout=cout: ops.conv3d_implicit(y, w, (n, 1, H, W), cout, _K3, _S1, _P1,  # noqa: E731
                                                                                   shift=b, relu=True)
                out[f"conv_{idx}"] = _stats(_time([f], a.warmup, a.steps)[0])
                y = f()
                if pool:
                    g = lambda y=y, H=H, W=W, cout=cout: ops.maxpool_fwd(y, n, cout, H, W, 2, 2, 0)  # noqa: E731
                    out[f"pool_{idx}"] = _stats(_time([g], a.warmup, a.steps)[0])
                    y = g()[0]
            y = y.view(n, -1)
            for i, (w, b) in zip((0, 2, 4), pk["fcs"]):
                f = lambda y=y, w=w, b=b: ops.linear_fwd(y, w, b, epilogue=L.EPI_RELU)  # noqa: E731
                out[f"fc_{i}"] = _stats(_time([f], a.warmup, a.steps)[0])
                routes = {}
                for M in sorted({1, 32, n}):
                    plan = ops.gemm_plan(y[:M], w, M, w.shape[0], w.shape[1], a_kmajor=True, b_kmajor=True, lda=w.shape[1],
                                         ldb=w.shape[1], epilogue=L.EPI_RELU, bias=b)
                    routes[str(M)] = {"launch_bound": ops.gemm_is_launch_bound(M, w.shape[0], w.shape[1], dt),
                                      "kernel": plan.kernel, "split": plan.split}
                out[f"fc_{i}_route"] = routes
                y = f()
            out["expert"] = _stats(_time([lambda: net(wave)], a.warmup, a.steps)[0])

            # torch's own eager modules on the same examples
            features, emb = A.make_stack()
            sd = net.state_dict()
            features.load_state_dict({k[9:]: v for k, v in sd.items() if k.startswith("features.")})
            emb.load_state_dict({k[11:]: v for k, v in sd.items() if k.startswith("embeddings.")})
            features, emb = features.to(device="cuda", dtype=dt).eval(), emb.to(device="cuda", dtype=dt).eval()
            x = ex[:, None]

            def stack():
                z = features(x)
                return emb(z.permute(0, 2, 3, 1).reshape(n, -1))
            out["eager_stack"] = _stats(_time([stack], a.warmup, a.steps)[0])
            z = x
            for i, layer in enumerate(features):
                if not isinstance(layer, torch.nn.ReLU):
                    nxt = features[i + 1] if isinstance(layer, torch.nn.Conv2d) else (lambda t: t)
                    f = lambda z=z, layer=layer, nxt=nxt: nxt(layer(z))  # noqa: E731
                    out[f"eager_{'conv' if isinstance(layer, torch.nn.Conv2d) else 'pool'}_{i}"] = _stats(
                        _time([f], a.warmup, a.steps)[0])
                    z = f()
            z = z.permute(0, 2, 3, 1).reshape(n, -1)
            for i in (0, 2, 4):
                f = lambda z=z, i=i: emb[i + 1](emb[i](z))  # noqa: E731
                out[f"eager_fc_{i}"] = _stats(_time([f], a.warmup, a.steps)[0])
                z = f()
            got = net.embed(ex).float()
            out["rel_l2_vs_eager"] = float((got - z.float()).norm() / z.float().norm())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
