"""Plain torch-CPU statements of the row, gating, loss and LSTM-step kernels, their input builders and the tolerance rule
of tests/test_gpu_rowwise.py and tests/test_gpu_lstm.py.  No GPU is touched here; tests/test_rowwise_cpu.py checks this file.

Every operation is one function of tensors that works in whatever floating dtype it is handed:
  * ``ref64(op, *x)``      evaluates it in float64 -- the reference;
  * ``fp32_chain(op, *x)`` evaluates it in fp32 with one final rounding to the output dtype -- the arithmetic contract the
    kernels state (16-bit data widened to fp32, fp32 arithmetic, one rounding on the way out).
Operands are handed over already rounded to the kernel's dtype (the convention of tests/test_gpu_ops.py), so neither sees
an operand the kernel does not see.

The tolerance rule (``assert_close``).  The fp32 value a kernel forms may be off the float64 one by
    E = 4 * max|fp32 chain - float64| + ulp32(largest operand magnitude)
-- four times the fp32 chain's own worst error on these inputs (the margin tests/test_gpu_audio.py and
tests/test_gpu_lars.py use) plus one fp32 ulp of the largest magnitude that went into the tensor.  One huge element (a
clamped row's dy / eps, an fp16 operand of 6e4) must not buy slack for the small ones, so the same rule is also taken in
units of each element's own fp32 spacing -- with mag_i the largest magnitude behind element i (its operands and its
reference), w = max_j |chain_j - float64_j| / ulp32(mag_j), E_i = (4 w + 1) ulp32(mag_i) -- and an element gets the
smaller of the two.  An fp32 output must be within E_i of the reference.  A 16-bit output is that fp32 value rounded once,
so it must lie between the 16-bit rounding of (reference - E_i) and of (reference + E_i), widened by one representable
value on each side: where E_i is below the 16-bit spacing this is "the float64 result rounded to the dtype, or a
neighbouring representable value"."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as TF

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTYPE_ID = {"fp32": 0, "bf16": 1, "fp16": 2}            # DVT_F32 / DVT_BF16 / DVT_F16 of include/dvt_hip.h


# ---------------------------------------------------------------- evaluation in a chosen precision
def ref64(op, *xs, **kw):
    return op(*(None if x is None else x.double() for x in xs), **kw)


def fp32_chain(op, *xs, out_dtype=torch.float32, **kw):
    """the operation in torch CPU fp32, rounded once to ``out_dtype`` (tuples elementwise)"""
    out = op(*(None if x is None else x.float() for x in xs), **kw)
    if isinstance(out, tuple):
        return tuple(o.to(out_dtype) for o in out)
    return out.to(out_dtype)


def vjp(op, n_out=1):
    """the backward of ``op`` by autograd: (*inputs, *output gradients) -> input gradients (a tuple, or the one tensor)"""
    def bwd(*args, **kw):
        xs = [a.detach().clone().requires_grad_(True) for a in args[:len(args) - n_out]]
        gs = args[len(args) - n_out:]
        out = op(*xs, **kw)
        outs = out if isinstance(out, tuple) else (out,)
        grads = torch.autograd.grad(outs[:n_out], xs, gs, allow_unused=True)
        grads = tuple(torch.zeros_like(x) if g is None else g for g, x in zip(grads, xs))
        return grads if len(grads) > 1 else grads[0]
    return bwd


# ---------------------------------------------------------------- the operations
def cosine_rows(a, b, eps=1e-8):
    """nn.CosineSimilarity(dim=1, eps): each norm is clamped on its own"""
    na = a.square().sum(1).sqrt().clamp_min(eps)
    nb = b.square().sum(1).sqrt().clamp_min(eps)
    return (a * b).sum(1) / (na * nb)


def l2norm_rows(x, eps=1e-12):
    """F.normalize(x, dim=1, eps)"""
    return x / x.square().sum(1, keepdim=True).sqrt().clamp_min(eps)


def l2norm_inv(x, eps=1e-12):
    return 1.0 / x.square().sum(1).sqrt().clamp_min(eps)


def l2norm_rows_bwd(x, dy, eps=1e-12):
    """autograd of F.normalize: dy / eps on a clamped row (the zero row included)"""
    return vjp(lambda t: TF.normalize(t, dim=1, eps=eps))(x, dy)


def l2norm_rows_bwd_from_y(y, inv, dy, eps=1e-12):
    """the same gradient from what the backward kernel is handed (the stored y and 1 / max(||x||, eps)): the statement
    whose fp32 evaluation is the kernel's contract when y has already been rounded to 16 bits"""
    clamped = (inv >= 1.0 / eps).unsqueeze(1)
    return torch.where(clamped, inv.unsqueeze(1) * dy, inv.unsqueeze(1) * (dy - y * (y * dy).sum(1, keepdim=True)))


def gate(a, b):
    """F.glu(cat(x, x + x1), -1) with a = x, b = x + x1"""
    return a * torch.sigmoid(b)


gate_bwd = vjp(gate)                                    # (a, b, dy) -> (da, db)


def contrastive_rows(sim, temperature=0.5):
    """NT-Xent on a similarity matrix [2B, 2B] (tests/contrastive_ref.py ntxent): -> (loss, row_lse, row_loss);
    row_lse[k] = log sum_{j != k} exp(sim_kj / T), the positive of row k is column (k + B) mod 2B"""
    M = sim.shape[0]
    s = sim / temperature
    eye = torch.eye(M, dtype=torch.bool)
    lse = torch.logsumexp(s.masked_fill(eye, -math.inf), 1)
    pos = s[torch.arange(M), (torch.arange(M) + M // 2) % M]
    row = lse - pos
    return row.mean(), lse, row


def contrastive_dsim(sim, gloss, temperature=0.5):
    return vjp(lambda s: contrastive_rows(s, temperature)[0])(sim, gloss.reshape(()).to(sim.dtype))


def bce_logits(z, y):
    """F.binary_cross_entropy_with_logits(z, y) (mean)"""
    return (z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean()


def bce_logits_bwd(z, y, gloss):
    """(sigmoid(z) - y) gloss / n: the derivative torch's backward uses (autograd of the max / |z| form above is off at
    z = 0 exactly, where its pieces are not differentiable)"""
    return gloss.reshape(()).to(z.dtype) / z.numel() * (torch.sigmoid(z) - y)


def sigmoid_bce(z, y):
    """nn.BCELoss()(sigmoid(z), y): mean, each log term clamped at -100"""
    p = torch.sigmoid(z)
    return ((y - 1) * torch.log1p(-p).clamp_min(-100) - y * torch.log(p).clamp_min(-100)).mean()


def sigmoid_bce_bwd(z, y, gloss):
    """BCELoss's backward (the p (1 - p) denominator clamped at 1e-12) then sigmoid's, as torch evaluates them"""
    p = torch.sigmoid(z)
    pq = (1 - p) * p
    return gloss.reshape(()).to(z.dtype) / z.numel() * (p - y) / pq.clamp_min(1e-12) * pq


def ce_argmax(student, teacher):
    """F.cross_entropy(student, teacher.argmax(1)) (mean); the first maximum wins, an all -inf row gives index 0"""
    idx = teacher.argmax(1)
    return (torch.logsumexp(student, 1) - student[torch.arange(student.shape[0]), idx]).mean()


def ce_argmax_bwd(student, teacher, gloss):
    return vjp(lambda s: ce_argmax(s, teacher))(student, gloss.reshape(()).to(student.dtype))


ACT_GELU, ACT_RELU, ACT_SIGMOID = 1, 2, 3


def act(x, kind):
    if kind == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if kind == ACT_RELU:
        return x.clamp_min(0)
    return torch.sigmoid(x)


def act_bwd(x, dy, kind):
    """dy * act'(x): Phi(x) + x phi(x), 1[x > 0], s (1 - s)"""
    if kind == ACT_GELU:
        d = 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327
    elif kind == ACT_RELU:
        d = (x > 0).to(x.dtype)
    else:
        s = torch.sigmoid(x)
        d = s * (1 - s)
    return dy * d


def axpby(dst, src, alpha, beta):
    """dst = beta * dst + alpha * src; beta == 0 overwrites (a NaN or inf in dst is not propagated)"""
    return alpha * src if beta == 0 else beta * dst + alpha * src


def mean_rows(x, scale=None):
    return x.sum(1) * (1.0 / x.shape[1] if scale is None else scale)


def mean_rows_bwd(dout, Ln, scale=None):
    return (dout * (1.0 / Ln if scale is None else scale)).unsqueeze(1).expand(-1, Ln, -1).contiguous()


def rows_gather(src3, tok):
    """src3 [B, T, rows, d]: row 0 of every sequence, behind the token row where there is one -> [B, T (+1), d]"""
    out = src3[:, :, 0]
    if tok is not None:
        out = torch.cat([tok.to(out.dtype).reshape(1, 1, -1).expand(out.shape[0], 1, -1), out], 1)
    return out


def tokens_assemble_bwd(dout, T, pos_rows):
    """dout [S, n + 1, d] -> (demb [S n, d], dcls [d], dpos [T, pos_rows, d]); rows of dpos past n are zero"""
    S, n1, d = dout.shape
    demb = dout[:, 1:].reshape(S * (n1 - 1), d)
    dcls = dout[:, 0].sum(0)
    dpos = torch.zeros(T, pos_rows, d, dtype=dout.dtype)
    dpos[:, :n1] = dout.reshape(S // T, T, n1, d).sum(0)
    return demb, dcls, dpos


# ---------------------------------------------------------------- the tolerance rule
def ulp32(x):
    """spacing of fp32 at |x| (at least the smallest normal's)"""
    x = x.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def ordinal(t):
    """16-bit floats on an integer line on which neighbouring representable values differ by one (+-0 are both 0)"""
    assert t.dtype in (torch.bfloat16, torch.float16)
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))


def budget(ref, chain32, operand_mag):
    """E_i of the rule above: ``chain32`` is the fp32 chain before any 16-bit rounding, ``operand_mag`` the largest operand
    magnitude behind each element (a tensor broadcastable to ref, or a number)"""
    ref = ref.double()
    mag = torch.maximum(torch.as_tensor(operand_mag, dtype=torch.float64).abs().expand_as(ref), ref.abs())
    mag = torch.where(torch.isfinite(mag), mag, torch.full_like(mag, 3.0e38))
    err = (chain32.double() - ref).abs()
    ok = torch.isfinite(err)
    if not ok.any():
        return ulp32(mag)
    worst_abs = float(err[ok].max())
    worst_ulps = float((err[ok] / ulp32(mag[ok])).max())
    whole = 4.0 * worst_abs + float(ulp32(mag.max()))
    return torch.minimum(torch.full_like(mag, whole), (4.0 * worst_ulps + 1.0) * ulp32(mag))


def assert_close(got, ref, chain32, operand_mag, what=""):
    """the rule of this file's docstring; ``got`` is the kernel's output on the CPU, in its own dtype"""
    ref = ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert not torch.isnan(got.float()).any(), f"{what}: NaN in the output"
    E = budget(ref, chain32, operand_mag)
    if got.dtype == torch.float32:
        err = (got.double() - ref).abs()
        same_inf = torch.isinf(ref) & (got.double() == ref)
        bad = ~((err <= E) | same_inf)
    else:
        lo = ordinal((ref - E).to(got.dtype)) - 1
        hi = ordinal((ref + E).to(got.dtype)) + 1
        o = ordinal(got)
        bad = (o < lo) | (o > hi)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the budget; first at flat index {i}: "
                             f"got {float(got.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, "
                             f"E {float(E.flatten()[i]):.3e}")


# ---------------------------------------------------------------- input builders
def rounded(t, dtype):
    return t.to(dtype)


def l2norm_edge_rows(D, dtype, eps, gen):
    """[6, D] in ``dtype``: 0 a zero row; 1 a row with 0 < ||x|| < eps (where the dtype can hold one: its smallest
    subnormal is above 1e-8 in fp16, then the row repeats the zero row); 2 a row just above eps; 3 an ordinary row;
    4 (fp16) elements near 3e4, whose squares overflow fp16, otherwise a large ordinary row; 5 a one-hot row."""
    x = torch.zeros(6, D, dtype=torch.float64)
    u = torch.rand(D, generator=gen, dtype=torch.float64) + 0.5
    sgn = torch.where(torch.rand(D, generator=gen) < 0.5, -1.0, 1.0).double()
    x[1] = 0.25 * eps * u / u.norm() * sgn
    x[2] = 4.0 * eps * u / u.norm() * sgn
    x[3] = torch.randn(D, generator=gen, dtype=torch.float64)
    x[4] = (3.0e4 if dtype == torch.float16 else 3.0e3) * (0.9 + 0.1 * u / u.max()) * sgn
    x[5, D // 2] = -2.5
    out = x.to(dtype)
    if float(out[1].double().norm()) == 0.0 or float(out[1].double().norm()) >= eps:
        out[1] = 0
    return out


def cosine_small_norm_pair(dtype):
    """a = (3e-6, 4e-6, 0), b = (4e-6, 3e-6, 0): both norms are above eps = 1e-8 and their product is below it"""
    a = torch.tensor([[3e-6, 4e-6, 0.0]], dtype=torch.float64).to(dtype)
    b = torch.tensor([[4e-6, 3e-6, 0.0]], dtype=torch.float64).to(dtype)
    return a, b


def elementwise_values(n, dtype, gen, spread=3.0):
    """n values in ``dtype``: +-0, +-20, +-100 (and +-6e4 in fp16) first, as far as n reaches, then uniform ones in
    (-spread, spread).  Past |x| = 3 the fp32 GELU chain loses its relative accuracy to the cancellation in 1 + erf, so
    the ordinary values stop there; the specials are beyond it on both sides, where the chain is exact again."""
    special = [0.0, -0.0, 20.0, -20.0, 100.0, -100.0] + ([6.0e4, -6.0e4] if dtype == torch.float16 else [])
    x = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * spread
    k = min(n, len(special))
    x[:k] = torch.tensor(special[:k], dtype=torch.float64)
    return x.to(dtype)


CE_TIES = [(5, 64), (3, 67), (6, 70), (67, 130)]


def ce_case(rows, C, dtype, gen):
    """(student, teacher) [rows, C] in ``dtype``.  Every teacher row but the all -inf one has its maximum twice: at a pair
    of CE_TIES that fits C (in turn), else at (C // 4, C - 1) when C >= 3.  Lane = column mod 64, so in (5, 64) and
    (67, 130) the first maximum (lanes 5, 3) sits in a higher lane than the later equal one (lanes 0, 2): the cross-lane
    reduction has to prefer the lower column, not the lower lane; in (3, 67) and (6, 70) both are one lane's, whose own
    scan must keep the first.  Where rows >= 3, row 1 (never the last) is all -inf."""
    st = (torch.randn(rows, C, generator=gen, dtype=torch.float64) * 2).to(dtype)
    te = (torch.randn(rows, C, generator=gen, dtype=torch.float64)).to(dtype)
    top = float(te.double().max()) + 1.0
    k = 0
    for r in range(rows):
        if rows >= 3 and r == 1:
            te[r] = -math.inf
            continue
        fits = [p for p in CE_TIES if p[1] < C]
        pair = fits[k % len(fits)] if fits else ((C // 4, C - 1) if C >= 3 else None)
        k += 1
        if pair is not None:
            te[r, pair[0]] = top
            te[r, pair[1]] = top
    return st, te


def contrastive_sim(M, temperature, gen):
    """a similarity matrix [M, M] f32 with cosine-like entries; row 0 holds one entry with sim / T near 1000"""
    z = TF.normalize(torch.randn(M, 16, generator=gen, dtype=torch.float64))
    sim = (z @ z.T).float()
    sim[0, 1 % M] = 1000.0 * temperature
    return sim


# ---------------------------------------------------------------- LSTM recurrence
def lstm_recurrence(G, w_hh, b_ih, b_hh, B, T, *, h_dtype=None):
    """one nn.LSTM layer's chain in the precision of its arguments: G [B, T, 4H] = x W_ih^T -> (h [B, T, H],
    gates [B, T, 4H] post-activation (i, f, g, o), c [B, T, H]).  ``h_dtype``: h_t is rounded to it at every step (what
    the kernel writes and reads back) with a straight-through gradient, and so is the gradient of every step's
    pre-activations (the kernel's dG)."""
    H = w_hh.shape[1]
    G = G.reshape(B, T, 4 * H)
    h = torch.zeros(B, H, dtype=G.dtype)
    c = torch.zeros(B, H, dtype=G.dtype)
    hs, gs, cs = [], [], []
    for t in range(T):
        s = G[:, t] + h @ w_hh.T
        if b_ih is not None:
            s = s + b_ih
        if b_hh is not None:
            s = s + b_hh
        if h_dtype is not None and s.requires_grad:             # dG of a step is stored, and read back, in the 16-bit type
            s.register_hook(lambda g: g.to(h_dtype).to(g.dtype))
        i, f, g, o = s.split(H, 1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        if h_dtype is not None:
            h = h + (h.detach().to(h_dtype).to(h.dtype) - h.detach())
        hs.append(h); gs.append(torch.cat([i, f, g, o], 1)); cs.append(c)
    return torch.stack(hs, 1), torch.stack(gs, 1), torch.stack(cs, 1)


def lstm_dG(G, w_hh, b_ih, b_hh, B, T, dh_seq, dh_last, **kw):
    """gradient of the pre-activation gates: d/dG of <h, dh_seq> + <h[:, -1], dh_last>"""
    Gr = G.detach().clone().requires_grad_(True)
    h, _, _ = lstm_recurrence(Gr, w_hh, b_ih, b_hh, B, T, **kw)
    loss = 0
    if dh_seq is not None:
        loss = loss + (h * dh_seq.reshape(h.shape)).sum()
    if dh_last is not None:
        loss = loss + (h[:, -1] * dh_last).sum()
    return torch.autograd.grad(loss, Gr)[0].reshape(B * T, -1)


def lstm_step(G_t, h_prev, c_prev, w_hh, b_ih, b_hh):
    """one step from the state it is handed: -> (gates [B, 4H] post-activation, c_t, h_t before any rounding)"""
    H = w_hh.shape[1]
    s = G_t + h_prev @ w_hh.T
    if b_ih is not None:
        s = s + b_ih
    if b_hh is not None:
        s = s + b_hh
    i, f, g, o = s.split(H, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], 1), c, o * torch.tanh(c)


def lstm_bwd_chain(w_hh, gates, c, dh_seq, dh_last, *, store_dtype=None):
    """backward through time from the stored post-activation gates [B, T, 4H] and cell states [B, T, H]: -> dG [B T, 4H],
    the gradient of the pre-activation gates.  ``store_dtype``: dG of a step is rounded to it before the step below reads
    it (what the kernel stores and reads back); None keeps the exact chain."""
    B, T, H = c.shape
    dG = torch.zeros(B, T, 4 * H, dtype=c.dtype)
    dc = torch.zeros(B, H, dtype=c.dtype)
    for t in range(T - 1, -1, -1):
        dh = torch.zeros(B, H, dtype=c.dtype) if t == T - 1 else dG[:, t + 1] @ w_hh
        if dh_seq is not None:
            dh = dh + dh_seq.reshape(B, T, H)[:, t]
        if dh_last is not None and t == T - 1:
            dh = dh + dh_last
        i, f, g, o = gates[:, t].split(H, 1)
        cprev = c[:, t - 1] if t > 0 else torch.zeros_like(dc)
        tc = torch.tanh(c[:, t])
        dcv = dc + dh * o * (1 - tc * tc)
        dc = dcv * f
        step = torch.cat([dcv * g * i * (1 - i), dcv * cprev * f * (1 - f), dcv * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dG[:, t] = step if store_dtype is None else step.to(store_dtype).to(c.dtype)
    return dG.reshape(B * T, 4 * H)


def _ste_round(t, dtype):
    return t + (t.detach().to(dtype).to(t.dtype) - t.detach())


def lstm_layer_restated(x, w_ih, w_hh, b_ih, b_hh, gout, glast, dtype):
    """functional.lstm_layer restated in CPU fp32 with the kernel's roundings to ``dtype``: G = x W_ih^T, h_t at every
    step, dG at every step and dx; everything else fp32.  Operands arrive rounded.  -> (out, last, {gradients})"""
    B, T, _ = x.shape
    leaves = [t.detach().float().clone().requires_grad_(True) for t in (x, w_ih, w_hh, b_ih, b_hh)]
    xr, wi, wh, bi, bh = leaves
    G = _ste_round(xr.reshape(B * T, -1) @ wi.T, dtype)
    h, _, _ = lstm_recurrence(G, wh, bi, bh, B, T, h_dtype=dtype)
    ((h * gout.to(dtype).float()).sum() + (h[:, -1] * glast.to(dtype).float()).sum()).backward()
    grads = {"dx": xr.grad.to(dtype).float(), "dW_ih": wi.grad, "dW_hh": wh.grad, "db_ih": bi.grad, "db_hh": bh.grad}
    return h.detach(), h[:, -1].detach(), grads


# ---------------------------------------------------------------- the k-step case of the LSTM forward step
KSTEP_B, KSTEP_H = 17, 176       # a ragged second batch tile; five whole 32-wide chunks and a half one (wave 1's second)


def kstep_signs(B=KSTEP_B, H=KSTEP_H, seed=0):
    """rho [B] (+-1 per row), eps [H/8] (+-1 per 8-wide group), b [4H, H/8] (+-1): W_hh[o, 8q..8q+7] = eps[q] b[o, q] and
    the one open unit of group q in row r carries h_0 = rho[r] eps[q] tau, so output o of row r sums to
    n = rho[r] * sum_q b[o, q], kept within +-2 with every group contributing (b is never 0)."""
    gen = torch.Generator().manual_seed(seed)
    Q = H // 8
    rho = torch.where(torch.arange(B) % 3 == 1, -1, 1)
    eps = torch.where(torch.rand(Q, generator=gen) < 0.5, -1, 1)
    b = torch.empty(4 * H, Q, dtype=torch.int64)
    for o in range(4 * H):
        m = (o % 3 - 1) * 2                                     # row sums -2, 0, +2 in turn
        plus = (Q + m) // 2
        perm = torch.randperm(Q, generator=gen)
        row = -torch.ones(Q, dtype=torch.int64)
        row[perm[:plus]] = 1
        b[o] = row
    return rho, eps, b


def kstep_operands(dtype, B=KSTEP_B, H=KSTEP_H, seed=0):
    """(G [B * 2, 4H], w_hh [4H, H]) in ``dtype`` for a two-step run with no biases, and the integer sums n [B, 4H]"""
    rho, eps, b = kstep_signs(B, H, seed)
    Q = H // 8
    G = torch.zeros(B, 2, 4 * H, dtype=torch.float64)
    u = torch.arange(H)
    q = u // 8
    for r in range(B):
        is_open = (u % 8) == (r + q) % 8
        G[r, 0, 0:H] = 40.0                                     # i = 1
        G[r, 0, 2 * H:3 * H] = 40.0 * rho[r] * eps[q]           # g = +-1
        G[r, 0, 3 * H:] = torch.where(is_open, 40.0, -200.0)    # o = 1 or exactly 0
    w = (eps.unsqueeze(0) * b).repeat_interleave(8, 1).double()  # [4H, H]
    n = rho.unsqueeze(1) * b.sum(1).unsqueeze(0)                 # [B, 4H]
    return G.reshape(B * 2, 4 * H).to(dtype), w.to(dtype), n


def kstep_gates(n, tau):
    """float64 gates of step 1: (sigmoid, sigmoid, tanh, sigmoid)(tau n) over the four gate blocks"""
    s = tau * n.double()
    H = s.shape[1] // 4
    out = torch.sigmoid(s)
    out[:, 2 * H:3 * H] = torch.tanh(s[:, 2 * H:3 * H])
    return out


def kstep_faulty_sums(B=KSTEP_B, H=KSTEP_H, seed=0):
    """the sums n a faulty K loop would form, one [B, 4H] per fault: each 8-wide group, each 32-wide chunk and each
    wave's share (chunks w, w + 4, ...) dropped and doubled, and each group's h fragment paired with the next group's
    weights (a moved group)"""
    rho, eps, b = kstep_signs(B, H, seed)
    Q = H // 8
    base = rho.unsqueeze(1) * b.sum(1).unsqueeze(0)
    out = {}
    spans = {f"group{q}": [q] for q in range(Q)}
    spans.update({f"chunk{c}": list(range(4 * c, min(Q, 4 * c + 4))) for c in range((Q + 3) // 4)})
    spans.update({f"wave{w}": [q for q in range(Q) if (q // 4) % 4 == w] for w in range(4)})
    for name, qs in spans.items():
        part = rho.unsqueeze(1) * b[:, qs].sum(1).unsqueeze(0)
        out[f"drop_{name}"] = base - part
        out[f"double_{name}"] = base + part
    for q in range(Q):
        q2 = (q + 1) % Q
        # h of group q (rho eps[q] tau at its open unit) against the weights of group q2 (eps[q2] b[:, q2])
        moved = rho.unsqueeze(1) * (eps[q] * eps[q2] * b[:, q2]).unsqueeze(0)
        out[f"move_group{q}"] = base - rho.unsqueeze(1) * b[:, q].unsqueeze(0) + moved
    return base, out
