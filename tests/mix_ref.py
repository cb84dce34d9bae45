"""Plain torch-CPU statements of csrc/mix.hip: Mixup / CutMix of clips, the mixed targets and the soft-target cross-entropy,
each a function of tensors that works in the floating dtype it is handed, so that ``rowwise_ref.ref64`` evaluates it in
float64 (the reference) and ``rowwise_ref.fp32_chain`` in fp32 (the yardstick of ``rowwise_ref.assert_close``).  No GPU is
touched here; tests/test_mix_cpu.py checks this file.

The constants of a mix are the two fp32 numbers the kernel uses -- ``lam`` and ``oml = 1.0f - lam``, and for a label row
``off = smoothing / C`` and ``on = 1.0f - smoothing + off``, each formed in fp32 -- widened to the dtype of the evaluation."""
from __future__ import annotations

import torch

KIND_LEAVE, KIND_MIXUP, KIND_CUTMIX = 0, 1, 2


def fp32_pair(lam):
    """(lam, 1.0f - lam) as float32 tensors"""
    lam = torch.as_tensor(lam, dtype=torch.float32)
    return lam, torch.tensor(1.0, dtype=torch.float32) - lam


def changes(row, i, lam_i):
    """whether table row i changes its sample at all (what must stay bit-identical otherwise)"""
    partner, kind, t0, t1, y0, y1, x0, x1 = (int(v) for v in row)
    if partner == i or kind == KIND_LEAVE:
        return False
    if kind == KIND_MIXUP:
        return float(lam_i) != 1.0
    return t1 > t0 and y1 > y0 and x1 > x0


def clips_mix(x, table, lam):
    """x [B, T, C, H, W] in any floating dtype -> the mixed batch in that dtype, every read from the unmixed x"""
    table = torch.as_tensor(table, dtype=torch.int32).reshape(-1, 8)
    lam32, oml32 = fp32_pair(lam)
    out = x.clone()
    for i in range(x.shape[0]):
        row = table[i].tolist()
        if not changes(row, i, lam32[i]):
            continue
        p, kind, t0, t1, y0, y1, x0, x1 = row
        if kind == KIND_MIXUP:
            out[i] = lam32[i].to(x.dtype) * x[i] + oml32[i].to(x.dtype) * x[p]
        else:
            out[i, t0:t1, :, y0:y1, x0:x1] = x[p, t0:t1, :, y0:y1, x0:x1]
    return out


def label_rows(labels, C, smoothing, dtype):
    """smoothed one-hot rows [B, C]; a label outside [0, C) gives a NaN row"""
    s = torch.tensor(smoothing, dtype=torch.float32)
    off = s / torch.tensor(float(C), dtype=torch.float32)
    on = torch.tensor(1.0, dtype=torch.float32) - s + off
    rows = off.to(dtype).expand(labels.shape[0], C).clone()
    for r, l in enumerate(labels.tolist()):
        if 0 <= l < C:
            rows[r, l] = on.to(dtype)
        else:
            rows[r] = float("nan")
    return rows


def targets_mix(t, table, lam):
    """t [B, C] (multi-hot rows or ``label_rows``) -> lam t + oml t[partner]; a row with lam == 1 is its own target"""
    table = torch.as_tensor(table, dtype=torch.int32).reshape(-1, 8)
    lam32, oml32 = fp32_pair(lam)
    partner = table[:, 0].long()
    mixed = lam32.to(t.dtype).unsqueeze(1) * t + oml32.to(t.dtype).unsqueeze(1) * t[partner]
    return torch.where((oml32 == 0).unsqueeze(1), lam32.to(t.dtype).unsqueeze(1) * t, mixed)


def ce_soft(x, t):
    """-> (loss, lse [M], tsum [M]): mean over the rows of sum_c -t_c (x_c - lse)"""
    lse = torch.logsumexp(x, 1)
    return (t * (lse.unsqueeze(1) - x)).sum(1).mean(), lse, t.sum(1)


def ce_soft_bwd(x, t, lse, tsum, gloss):
    """dx = g / M (softmax(x) sum_c t_c - t), from the saved lse and target sums"""
    return gloss.reshape(()).to(x.dtype) / x.shape[0] * (torch.exp(x - lse.unsqueeze(1)) * tsum.unsqueeze(1) - t)
