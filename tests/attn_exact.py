"""Attention operands whose softmax is exact, and the float64 reference of their forward and backward.

Every (b, h) draws its own small-integer Q, K, V, dO (exact in bf16 and fp16).  The scores are built from channels:
  channel 0 (bias):     Q = 1, K = -A on every real key
  channel 1 + g:        Q = 1 on the rows that select key group g, K = A on the keys of group g
  (graded) channel cm:  Q = m_i (the row's offset), K = 1 on every real key
  (graded) channel ct:  Q = 1, K = -t_j (t_j in {0, 1})
  the rest:             "free" channels, small integers in Q only or in K only (they never touch a score)
so row i scores the keys of its group at m_i - t_j and every other real key A lower.  A padded key (j >= Lk) has a zero K
row and scores exactly 0.

tied   scale 0.125, A = 8192, m = t = 0, group sizes powers of two: each row's selected keys score 0 (the row maximum, which
       a padded key shares: a missing mask changes l), the others -1024 after scaling (probability exactly 0 in fp32);
       probabilities are 0 or 1/n.
graded scale with fp32(scale * log2 e) == 1 (the MFMA kernels' exp2 argument is then the integer score minus the row
       maximum), A = 4096, row offsets m_i from -8 to 140 (a kernel without the subtract-max step overflows at 2^130),
       t_j in {0, 1} chosen so each group's weights sum to a power of two.
"""
import math

import numpy as np
import torch

SCALE_TIED = 0.125
SCALE_GRADED = 0.6931471824645996
F64 = torch.float64


def graded_scale_ok():
    """fp32(scale) * fp32(log2 e) rounds to exactly 1.0 in fp32 (the kernels' c2 = scale * kLog2e)"""
    s = np.float32(SCALE_GRADED)
    return float(s) == SCALE_GRADED and np.float32(s * np.float32(1.4426950408889634)) == np.float32(1.0)


def _groups(Lk, G, pow2, rng):
    """sizes of key groups covering Lk keys: powers of two (tied) or any; split the largest until there are G"""
    sizes = [1 << b for b in range(Lk.bit_length()) if Lk >> b & 1] if pow2 else [Lk]
    while len(sizes) < G and max(sizes) >= 2:
        sizes.sort()
        s = sizes.pop()
        sizes += [s // 2, s - s // 2]
    rng.shuffle(sizes)
    return sizes


def channel_plan(Lq, Lk, dh, mode):
    """number of key groups and the channel layout for these sizes"""
    extra = 2 if mode == "graded" else 0
    free = max(4, dh // 3)
    G = max(1, min(Lq, dh - 1 - extra - free, 24))
    return G, extra


def head_operands(Lq, Lk, dh, mode, rng):
    """(q, k, v, do) float64 of one (b, h), plus the key groups of each row"""
    G, extra = channel_plan(Lq, Lk, dh, mode)
    tied = mode == "tied"
    A = 8192.0 if tied else 4096.0
    sizes = _groups(Lk, G, tied, rng)
    G = len(sizes)
    perm = rng.permutation(Lk)
    grp = np.empty(Lk, dtype=np.int64)
    o = 0
    for g, s in enumerate(sizes):
        grp[perm[o:o + s]] = g
        o += s
    # every group is selected by at least one row; the remaining rows pick at random
    assert G <= Lq, "more key groups than query rows"
    sel = np.concatenate([rng.permutation(G), rng.integers(0, G, Lq - G)])
    rng.shuffle(sel)
    q = np.zeros((Lq, dh))
    k = np.zeros((Lk, dh))
    q[:, 0] = 1.0
    k[:, 0] = -A
    q[np.arange(Lq), 1 + sel] = 1.0
    k[np.arange(Lk), 1 + grp] = A
    c0 = 1 + G
    if not tied:
        cm, ct = c0, c0 + 1
        c0 += 2
        m = rng.integers(-8, 9, Lq).astype(np.float64)
        if Lq > 1:                               # (a single row keeps a small maximum: the padded keys stay visible)
            big = rng.choice(Lq, size=max(1, Lq // 8), replace=False)
            m[big] = rng.integers(100, 141, big.size)
            m[big[0]] = 140
        q[:, cm] = m
        k[:, cm] = 1.0
        t = np.ones(Lk)
        for g, s in enumerate(sizes):            # D = 2^ceil(log2 s) - s keys weigh 2, the rest 1: the weights sum to 2^e
            keys = np.nonzero(grp == g)[0]
            D = (1 << (s - 1).bit_length()) - s
            t[rng.permutation(keys)[:D]] = 0.0
        q[:, ct] = 1.0
        k[:, ct] = -t
    free = np.arange(c0, dh)
    qf, kf = free[0::2], free[1::2]
    # sparse small integers: one or two free channels per row / key
    for mat, ch, n in ((q, qf, Lq), (k, kf, Lk)):
        if ch.size:
            for r in range(n):
                c = rng.choice(ch, size=min(2, ch.size), replace=False)
                mat[r, c] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=c.size)
    v = np.where(rng.random((Lk, dh)) < 0.25, rng.integers(-2, 3, (Lk, dh)), 0).astype(np.float64)
    draw = lambda n: np.where(rng.random((n, dh)) < 0.08, rng.choice([-1.0, 1.0], (n, dh)), 0.0)
    do = draw(Lq)
    fix_gradients(q, k, v, do, sel, tied, draw, rng)
    return q, k, v, do


def _fits16(x):
    """every value survives a round trip through bf16 and through fp16"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    return all(torch.equal(t.to(d).double(), t) for d in (torch.bfloat16, torch.float16))


def fix_gradients(q, k, v, do, sel, tied, draw, rng):
    """Redraw (in the end: zero) rows of dO until dS = P (dP - delta) fits both 16-bit types (the MFMA backward rounds dS to
    16 bits) and, in tied mode (scale a power of two), dQ and dK fit them too.  dS and dQ of row i depend on dO_i alone;
    dK of a key depends on the dO rows of the rows that select its group."""
    scale = SCALE_TIED if tied else SCALE_GRADED
    s = q @ k.T
    s = s - s.max(1, keepdims=True)
    e = np.exp(s * SCALE_TIED) if tied else np.exp2(s)
    p = e / e.sum(1, keepdims=True)
    o = p @ v

    def row_ok(i):
        ds = p[i] * (v @ do[i] - do[i] @ o[i])
        return _fits16(ds) and (not tied or _fits16(scale * (ds @ k)))

    def redraw(i):
        for _ in range(20):
            do[i] = draw(1)[0]
            if row_ok(i):
                return
        do[i] = 0.0

    for i in range(len(q)):
        if not row_ok(i):
            redraw(i)
    if not tied:
        return
    for g in range(sel.max() + 1):
        rows = np.nonzero(sel == g)[0]
        for _ in range(4 * len(rows) + 20):
            ds = p[rows] * (do[rows] @ v.T - (do[rows] * o[rows]).sum(1, keepdims=True))
            if _fits16(scale * (ds.T @ q[rows])):
                break
            live = rows[np.abs(do[rows]).sum(1) > 0]
            i = rng.choice(live)
            redraw(i)
            if rng.random() < 0.25:
                do[i] = 0.0


def operands(B, H, Lq, Lk, dh, mode, seed):
    """float64 [B, H, L, dh] q, k, v, do; every (b, h) its own draw"""
    rng = np.random.default_rng(seed)
    parts = [head_operands(Lq, Lk, dh, mode, rng) for _ in range(B * H)]
    out = []
    for i, L in enumerate((Lq, Lk, Lk, Lq)):
        out.append(torch.from_numpy(np.stack([p[i] for p in parts])).reshape(B, H, L, dh))
    return tuple(out)


def scale_of(mode):
    return SCALE_TIED if mode == "tied" else SCALE_GRADED


def reference(q, k, v, do, scale, graded=False, Lk_admit=None):
    """float64 forward and backward: dict o, lse, delta, p, ds, dq, dk, dv and the magnitudes |.| of each gradient's terms
    (bounds of what an inexact probability can move).  graded: probabilities 2^(s - max) of the integer scores s (what
    fp32(scale * log2 e) == 1 makes of them), gradients scaled by `scale`.  Lk_admit: also admit that many zero (padded)
    keys."""
    if Lk_admit:
        z = torch.zeros(*k.shape[:2], Lk_admit, k.shape[3], dtype=F64)
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    s = q @ k.transpose(-1, -2)
    if not graded:
        s = s * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m) if graded else torch.exp(s - m)
    lsum = e.sum(-1, keepdim=True)
    p = e / lsum
    o = p @ v
    lse = ((m + torch.log2(lsum)) * math.log(2.0) if graded else m + torch.log(lsum)).squeeze(-1)
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(-1, -2) @ q)
    dv = p.transpose(-1, -2) @ do
    if Lk_admit:                                  # gradients of the real keys only
        dk, dv = dk[:, :, :-Lk_admit], dv[:, :, :-Lk_admit]
    ads = p * (dp.abs() + delta.abs())
    mag = dict(o=p @ v.abs(), dq=scale * (ads @ k.abs()), dk=scale * (ads.transpose(-1, -2) @ q.abs()),
               dv=p.transpose(-1, -2) @ do.abs())
    return dict(o=o, lse=lse, delta=delta.squeeze(-1), p=p, ds=ds, dq=dq, dk=dk, dv=dv, mag=mag)


def representable(x, dtype):
    """every value of the float64 tensor x survives a round trip through dtype"""
    return bool(torch.equal(x.to(dtype).to(F64), x)) and bool(torch.isfinite(x.to(dtype)).all())


def ulp(x, dtype):
    """one unit in the last place of dtype at |x| (the spacing above |x|), per element, in float64"""
    fi = torch.finfo(dtype)
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dtype]
    ax = x.abs().clamp_min(fi.tiny)
    e = torch.floor(torch.log2(ax))
    return torch.pow(2.0, e - mant).to(F64)


def mismatch(got, ref, dtype, exact, mag=None, rel=0.0, ulps=1):
    """bool mask of elements that fail: where `exact` (a bool mask or True) got must equal ref rounded once to dtype;
    elsewhere |got - ref| <= ulps ulp(ref) + rel * mag"""
    got = got.to(F64)
    want = ref.to(dtype).to(F64)
    tol = ulps * ulp(ref, dtype)
    if mag is not None:
        tol = tol + rel * mag
    bad = ((got - ref).abs() > tol) | torch.isnan(got)
    if exact is True:
        bad = bad | (got != want)
    elif exact is not False:
        bad = bad | (exact & (got != want))
    return bad


# ------------------------------------------------------------------ cases
# id -> geometry (B, H, Lq, Lk, dh), operand mode, layout ("packed": the [B, tokens, 3, H, dh] buffer the blocks use;
# "skew": head stride dh + 1, no multiple of 8), two_pass, dtypes.  The plan each case takes is asserted by the GPU test
# and its kernel symbols are gated by tests/test_attention_coverage.py.
_16 = ("bf16", "fp16")


def _c(B, H, Lq, Lk, dh=64, mode="tied", layout="packed", two_pass=False, dtypes=_16):
    return dict(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, mode=mode, layout=layout, two_pass=two_pass, dtypes=dtypes)


CASES_BASE = {
    # register-resident forward res<E, 1..7> with the one-pass backward fused<E, 1..7>; 32k + 1 and 32k lengths
    "L17": _c(2, 2, 17, 17),
    "L64": _c(1, 3, 64, 64),
    "L65": _c(2, 2, 65, 65),
    "L97_graded": _c(2, 2, 97, 97, mode="graded"),
    "L160": _c(1, 2, 160, 160),
    "L161": _c(1, 2, 161, 161),
    "q193_k224": _c(1, 2, 193, 224),
    "q224_k193_graded": _c(1, 2, 224, 193, mode="graded"),
    # res<E, 8..11> with the kernel pair dq<E, n> / dkv<E, n>; both store modes of res 9
    "L225": _c(1, 2, 225, 225),
    "L257_graded": _c(1, 2, 257, 257, mode="graded"),
    "L289": _c(1, 2, 289, 289),
    "q40_k289": _c(1, 2, 40, 289),
    "q40_k257": _c(2, 2, 40, 257),
    "q150_k250": _c(1, 2, 150, 250),
    # long query side, short key side: dkv<E, 8> / dkv<E, 9> with LDS-patch stores
    "q240_k40": _c(1, 2, 240, 40),
    "q257_k20": _c(2, 2, 257, 20),
    "L320": _c(1, 2, 320, 320),
    "L352": _c(1, 2, 352, 352),
    # online forward (> 352 keys, up to the LDS limit of 640) and the rolled loops dq<E, 0> / dkv<E, 0>
    "L353": _c(1, 2, 353, 353),
    "L608_graded": _c(1, 2, 608, 608, mode="graded"),
    "q40_k640": _c(1, 2, 40, 640),
    "q40_k600": _c(1, 2, 40, 600),
    # two_pass: the pair at lengths the one-pass backward would take
    "L17_pair": _c(2, 2, 17, 17, two_pass=True),
    "L33_pair": _c(2, 2, 33, 33, two_pass=True),
    "L96_pair": _c(1, 2, 96, 96, two_pass=True),
    "L97_pair": _c(1, 2, 97, 97, two_pass=True),
    "L129_pair": _c(1, 2, 129, 129, two_pass=True),
    "L161_pair": _c(1, 2, 161, 161, two_pass=True),
    "L193_pair_graded": _c(1, 2, 193, 193, two_pass=True, mode="graded"),
    # one query per (b, h)
    "q1_k256": _c(2, 2, 1, 256),
    "q1_k100_graded": _c(2, 2, 1, 100, mode="graded"),
    # short sequences: the small kernels at 256 and 512 threads (16-bit: dh != 64)
    "small_dh32": _c(2, 2, 24, 24, dh=32, dtypes=_16 + ("fp32",)),
    "small_dh128": _c(1, 2, 32, 32, dh=128, dtypes=_16 + ("fp32",)),
    "small_dh48_graded": _c(2, 2, 17, 31, dh=48, mode="graded", dtypes=_16 + ("fp32",)),
    # generic kernels: a head stride that is no multiple of 8 at dh = 64, dh = 96 with L = 40, Lk > 640
    "gen_skew": _c(1, 2, 33, 33, layout="skew", dtypes=_16 + ("fp32",)),
    "gen_dh96": _c(1, 2, 40, 40, dh=96, dtypes=_16 + ("fp32",)),
    "gen_k700": _c(1, 2, 40, 700),
    "gen_fp32_L64": _c(1, 2, 64, 64, dtypes=("fp32",)),
    "gen_fp32_L65_graded": _c(1, 2, 65, 65, mode="graded", dtypes=("fp32",)),
}
CASES = {f"{k}-{d}": dict(v, dtype=d) for k, v in CASES_BASE.items() for d in v["dtypes"]}
TORCH_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def seed_of(cid):
    c = CASES[cid]
    return c["Lq"] * 1009 + c["Lk"] * 31 + c["dh"] + (7 if c["mode"] == "graded" else 0)


def layout(c, dtype, device, fill=float("nan")):
    """(buffer, [q, k, v] views) of a packed [B, Lbuf, 3, H + 1, dhb] buffer; "skew" pads dh by one element"""
    B, H, Lq, Lk, dh = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"]
    dhb = dh + 1 if c["layout"] == "skew" else dh
    buf = torch.full((B, max(Lq, Lk) + 1, 3, H + 1, dhb), fill, dtype=dtype, device=device)
    views = [buf[:, :L, i, :H, :dh].permute(0, 2, 1, 3) for i, L in enumerate((Lq, Lk, Lk))]
    return buf, views


def out_layout(c, dtype, device, fill=float("nan")):
    """(buffer, view) of a [B, Lq + 1, H + 1, dhb] buffer: the O / dO layout"""
    B, H, Lq, dh = c["B"], c["H"], c["Lq"], c["dh"]
    dhb = dh + 1 if c["layout"] == "skew" else dh
    buf = torch.full((B, Lq + 1, H + 1, dhb), fill, dtype=dtype, device=device)
    return buf, buf[:, :Lq, :H, :dh].permute(0, 2, 1, 3)


def inside(buf, take):
    """bool mask of the elements of buf that the view `take(buf)` covers"""
    idx = torch.arange(buf.numel(), device=buf.device).view(buf.shape)
    m = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    m[take(idx).reshape(-1)] = True
    return m.view(buf.shape)


_ELEM = {"bf16": "std::bfloat16_t", "fp16": "_Float16", "fp32": "float"}


def fwd_symbols(fwd, dname):
    """demangled kernel names (without the namespace and parameter list) a forward plan launches"""
    E = _ELEM[dname]
    return {"q1": [f"attn_fwd_q1_kernel<{E}>"], "res": [f"attn_fwd_mfma_res_kernel<{E}, {fwd.count}>"],
            "online": [f"attn_fwd_mfma_kernel<{E}>"], "small": [f"attn_small_fwd_kernel<{E}>"],
            "generic": [f"attn_fwd_generic_kernel<{E}>"]}[fwd.family]


def bwd_symbols(bwd, dname):
    """the same for a backward plan (the pair: dq, then dk/dv)"""
    E = _ELEM[dname]
    return {"q1": [f"attn_bwd_q1_kernel<{E}>"], "fused": [f"attn_bwd_fused_kernel<{E}, {bwd.count}>"],
            "pair": [f"attn_bwd_dq_mfma_kernel<{E}, {bwd.count}>", f"attn_bwd_dkv_mfma_kernel<{E}, {bwd.count2}>"],
            "small": [f"attn_small_bwd_kernel<{E}>"],
            "generic": [f"attn_delta_kernel<{E}>", f"attn_bwd_dq_generic_kernel<{E}>",
                        f"attn_bwd_dkv_generic_kernel<{E}>"]}[bwd.family]


def plan_symbols(fwd, bwd, dname):
    return fwd_symbols(fwd, dname) + bwd_symbols(bwd, dname)


def plans(cid, device="cpu"):
    """(forward plan, backward plan) the case's views take (no launch)"""
    from dvt_amd import ops
    c = CASES[cid]
    dt = TORCH_DTYPES[c["dtype"]]
    _, (q, k, v) = layout(c, dt, device, fill=0.0)
    _, o = out_layout(c, dt, device, fill=0.0)
    scale = scale_of(c["mode"])
    return (ops.attention_plan(q, k, v, o, scale=scale),
            ops.attention_plan(q, k, v, o, bwd=True, do=o, two_pass=c["two_pass"], scale=scale))
