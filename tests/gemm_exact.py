"""Integer operands on which a GEMM kernel cannot be subtly wrong unseen: for the exact tests of the GEMM family
(tests/test_gpu_gemm_exact.py) and the CPU proof that they are sensitive (tests/test_gemm_coverage.py).

C[m, n] = sum_k A(m, k) B(k, n).  One operand is sparse: per row and per `chunk`-wide k range (16 wide unless K is deep)
exactly one nonzero, at a pseudo-random position, of magnitude 1 or 2 and a sign that flips every two ranges (so that no
32-wide step cancels itself).  The other operand is dense with values 1, 2, 3, pseudo-random along k and along its rows.  So
  * every product and every partial sum is a small integer: exact in fp32 in any order of addition, split-K slabs included;
  * every k range adds a nonzero amount to every output (with 16-wide ranges: every 16- and 32-wide k-step does);
  * which position of a range holds the nonzero changes the output: a swizzle slip inside a k-tile is seen;
  * rows and columns of C differ: a transposed, shifted or duplicated tile is seen;
  * the alternating signs keep the outputs small, so they are exact in the output type (checked, `check_bound`).
Deep K takes wider ranges (at most 64 of them), never an fp32 output.

Epilogue operands are integers too (bias, residual, the DRELU mask, accumulate's prior contents); DGELU's aux is taken from
the 16-bit grid (its product with an exact sum is exact in fp32 and rounds once); alpha is a power of two.  GELU forward is
the only transcendental: its pre-activation is exact and kept in [-3.5, 3.5], where the epilogue's erf approximation
(absolute error 1.5e-7) is within one ulp of bf16 / fp16, so output and saved derivative are compared with float64 within
one ulp of the output type.
"""
import math

import torch

LIMIT = {torch.bfloat16: 256, torch.float16: 2048, torch.float32: 2 ** 24 - 1}
CANARY = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A, torch.float32: 0x7FC0BEEF}   # NaN payloads no kernel computes
_IVIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def chunk_for(K):
    """range width: 16, doubled until there are at most 64 ranges"""
    c = 16
    while -(-K // c) > 64:
        c *= 2
    return c


def sparse_rows(rows, K, seed, chunk=None):
    """[rows, K] float64: one nonzero per `chunk`-wide k range and row (the last range may be short)"""
    chunk = chunk or chunk_for(K)
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(rows, K, dtype=torch.float64)
    r = torch.arange(rows)
    for c in range(-(-K // chunk)):
        lo, hi = c * chunk, min(K, (c + 1) * chunk)
        pos = lo + torch.randint(0, hi - lo, (rows,), generator=g)
        mag = 1.0 + torch.randint(0, 2, (rows,), generator=g).double()
        x[r, pos] = -mag if (c // 2) % 2 else mag
    return x


def dense(rows, K, seed):
    """[rows, K] float64 with values 1, 2, 3"""
    g = torch.Generator().manual_seed(seed)
    return 1.0 + torch.randint(0, 3, (rows, K), generator=g).double()


def operands(M, N, K, seed):
    """logical (A [M, K], B [K, N]) float64: A sparse along k, B dense"""
    return sparse_rows(M, K, seed), dense(N, K, seed + 1).t()


def small_ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def grid16(shape, dtype, seed):
    """float64 values on the 16-bit grid of `dtype`, magnitudes 1/8 .. 2 (a saved GELU derivative)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 1.875 + 0.125).to(dtype).double()


def check_bound(ref, dtype):
    """the outputs are exact integers (times alpha) within the range where `dtype` holds them exactly"""
    lim = LIMIT[dtype]
    assert ref.abs().max() <= lim, f"operands leave the exact range of {dtype}: max |C| = {float(ref.abs().max())} > {lim}"
    assert torch.equal(ref.to(dtype).double(), ref), f"an exact output is not representable in {dtype}"


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ulp(ref, dtype):
    """spacing of `dtype` at |ref| (float64 tensor)"""
    q = ref.to(dtype)
    if dtype == torch.float32:
        nxt = torch.nextafter(q.abs(), torch.tensor(float("inf"), dtype=dtype))
    else:
        nxt = (q.abs().view(torch.int16) + 1).view(dtype)
    return (nxt.double() - q.abs().double()).abs()


def epilogue64(acc, epi, *, alpha=1.0, bias=None, residual=None, aux=None):
    """float64 epilogue of dvt_gemm: -> (C, pre-activation for GELU else None)"""
    v = acc * alpha
    b = bias.view(1, -1) if bias is not None else 0.0
    if epi == 0:
        return v + b, None
    if epi == 1:
        return gelu64(v + b), v + b
    if epi == 2:
        return torch.clamp(v + b, min=0.0), None
    if epi == 3:
        return v + b + residual, None
    if epi == 4:
        return v * aux, None
    if epi == 5:
        return torch.where(aux > 0, v, torch.zeros_like(v)), None
    raise ValueError(epi)


def layout(x, kmajor_rows, dtype, device, *, pad=8, offset=8, lead_rows=1):
    """store the logical operand `x` ([mn, k] when kmajor_rows else [k, mn]: the storage's rows) in a buffer with `pad`
    spare columns and `lead_rows` spare rows in front, as a view that starts `lead_rows` rows and `offset` elements in:
    -> (view, ld)"""
    rows, cols = x.shape
    ld = cols + pad
    buf = torch.zeros(rows + lead_rows + 1, ld + offset, dtype=dtype, device=device)
    ld = buf.stride(0)
    view = buf[lead_rows:lead_rows + rows, offset:offset + cols]
    view.copy_(x.to(dtype))
    return view, ld


def canaried(M, N, dtype, device, *, pad=8, spare=3, fill=None):
    """C with ldc = N + pad and `spare` rows past M, all filled with CANARY bits; [M, N] holds `fill` (NaN unless given)
    -> (buffer, view)"""
    buf = torch.empty(M + spare, N + pad, dtype=dtype, device=device)
    buf.view(_IVIEW[dtype]).fill_(CANARY[dtype])
    view = buf[:M, :N]
    if fill is None:
        view.fill_(float("nan"))
    else:
        view.copy_(fill.to(dtype))
    return buf, view


def canaries_intact(buf, M, N):
    """every element of `buf` outside [M, N] still holds the canary bits -> number of overwritten ones"""
    iv = buf.view(_IVIEW[buf.dtype])
    c = CANARY[buf.dtype]
    mask = torch.ones_like(iv, dtype=torch.bool)
    mask[:M, :N] = False
    return int((iv[mask] != c).sum())


# ---------------------------------------------------------------- sensitivity (CPU): the faults these operands expose
def kstep_partials(A, B, step):
    """[(k0, partial product of the k range [k0, k0 + step))]: their sum is A @ B"""
    K = A.shape[1]
    return [(k0, A[:, k0:k0 + step] @ B[k0:k0 + step]) for k0 in range(0, K, step)]


def swapped_k(A, B, p, q):
    """A @ B with columns p and q of A swapped (one operand's element order slipped inside a k range)"""
    A2 = A.clone()
    A2[:, [p, q]] = A2[:, [q, p]]
    return A2 @ B


def shifted_fragment(C, i, j, di, dj):
    """C with the 16 x 16 output fragment at (16 i, 16 j) replaced by the one at (16 (i + di), 16 (j + dj))"""
    D = C.clone()
    D[16 * i:16 * i + 16, 16 * j:16 * j + 16] = C[16 * (i + di):16 * (i + di) + 16, 16 * (j + dj):16 * (j + dj) + 16]
    return D
