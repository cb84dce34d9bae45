"""Exact tests of every attention kernel (csrc/attention.hip) on operands whose softmax is exact (tests/attn_exact.py).

Each case asserts the plan dvt_attention_plan reports for its views, runs the forward and the backward (twice: bitwise
reproducible) with O, dQ, dK, dV written as views into NaN-filled buffers whose padding -- rows past the sequence, the
other two thirds of the packed [tokens, 3, H, dh] layout, a further head's columns -- carries canary values, and lse and
the workspace canaried past their end.  Outputs are compared with the float64 reference: equal to it rounded once to
the output type wherever the kernel's arithmetic is exact on these operands, within one ulp (plus the bound of an
inexact natural exponential, where the kernel takes one) elsewhere."""
import ctypes as C

import pytest
import torch

from tests import attn_exact as X

pytestmark = pytest.mark.gpu

CANARY = -29.0          # exact in every type, never an output of these operands
# families whose probabilities come from exp2 of the integer score (c2 == 1 in graded mode, 0 / 1/n in tied mode)
MFMA = ("res", "online", "fused", "pair")


def _rel(family, dname):
    """relative bound of the natural-exp kernels' inexact probabilities (0: the arithmetic is exact on these operands)"""
    return 0.0 if family in MFMA else 3e-5       # expf of a scaled score of up to ~100: a few fp32 ulps of the exponent


def _check(name, got, ref, mag, dtype, family, dname, exact_model):
    rel = _rel(family, dname)
    ul = X.ulp(ref, dtype)
    repr_ = ref.to(dtype).to(X.F64) == ref
    if not exact_model:
        exact = torch.zeros_like(repr_)
    elif rel == 0:                                # exp2 kernels: the builder makes every output representable
        assert bool(repr_.all()), f"{name}: reference not representable in {dtype}"
        exact = True
    else:                                         # natural exp: exact wherever the bound keeps the rounding
        exact = repr_ & (rel * mag <= ul / 4)
    bad = X.mismatch(got, ref, dtype, exact, mag=mag, rel=rel, ulps=1)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {list(i)}: "
                             f"got {float(got[i])}, want {float(ref[i])}")


def _canaried_flat(n, dtype, device, extra=64):
    buf = torch.full((n + extra,), CANARY, dtype=dtype, device=device)
    buf[:n] = float("nan")
    return buf


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _canaries_ok(buf, inner):
    """the elements of buf outside the mask `inner` still hold CANARY, bit for bit"""
    want = torch.full_like(buf, CANARY)
    return bool(torch.equal(_bits(buf)[~inner], _bits(want)[~inner]))


def run_case(cid, device):
    from dvt_amd import ops
    import dvt_amd
    c = X.CASES[cid]
    dname = c["dtype"]
    dtype = X.TORCH_DTYPES[dname]
    B, H, Lq, Lk, dh, mode = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["mode"]
    graded = mode == "graded"
    scale = X.scale_of(mode)
    q64, k64, v64, do64 = X.operands(B, H, Lq, Lk, dh, mode, X.seed_of(cid))
    ref = X.reference(q64, k64, v64, do64, scale, graded=graded)

    qkv_buf, (q, k, v) = X.layout(c, dtype, device, fill=CANARY)
    for view, val in ((q, q64), (k, k64), (v, v64)):
        view.copy_(val.to(dtype))
    o_buf, o = X.out_layout(c, dtype, device, fill=CANARY)
    o.fill_(float("nan"))
    do_buf, do = X.out_layout(c, dtype, device, fill=CANARY)
    do.copy_(do64.to(dtype))
    lse_buf = _canaried_flat(B * H * Lq, torch.float32, device)
    n_lse = B * H * Lq

    fwd_plan, bwd_plan = X.plans(cid)
    assert ops.attention_plan(q, k, v, o, scale=scale) == fwd_plan
    assert ops.attention_plan(q, k, v, o, bwd=True, do=do, two_pass=c["two_pass"], scale=scale) == bwd_plan

    lse = ops.attention_fwd(q, k, v, o, scale, lse=lse_buf[:n_lse])
    torch.cuda.synchronize()
    in_o = X.inside(o_buf, lambda t: t[:, :Lq, :H, :dh])
    assert _canaries_ok(o_buf, in_o), "forward wrote outside O"
    assert torch.equal(_bits(lse_buf[n_lse:]), _bits(torch.full_like(lse_buf[n_lse:], CANARY))), "forward wrote past lse"
    got_o = o.double().cpu()
    assert not got_o.isnan().any(), f"O: {int(got_o.isnan().sum())} elements never written"
    _check("O", got_o, ref["o"], ref["mag"]["o"], dtype, fwd_plan.family, dname, True)
    lse_ref = ref["lse"].reshape(-1)
    tol = 4 * X.ulp(lse_ref.abs().clamp_min(1.0), torch.float32)
    lse_err = (lse.double().cpu().reshape(-1) - lse_ref).abs()
    assert bool((lse_err <= tol).all()), f"lse off by up to {float(lse_err.max())}"

    lib = dvt_amd._lib.load()
    outs = []
    for rep in range(2):
        g_buf, (dq, dk, dv) = X.layout(c, dtype, device, fill=CANARY)
        for t in (dq, dk, dv):
            t.fill_(float("nan"))
        need = lib.dvt_attention_bwd_workspace_bytes(C.byref(ops._attn_desc(q, k, v, o, lse, scale)))
        ws_buf = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=device)
        ops.attention_bwd(q, k, v, o, lse, do, dq, dk, dv, scale, two_pass=c["two_pass"], ws=ws_buf[:need])
        torch.cuda.synchronize()
        in_g = X.inside(g_buf, lambda t: t[:, :Lq, 0, :H, :dh]) | X.inside(g_buf, lambda t: t[:, :Lk, 1, :H, :dh]) | \
            X.inside(g_buf, lambda t: t[:, :Lk, 2, :H, :dh])
        assert _canaries_ok(g_buf, in_g), "backward wrote outside dQ / dK / dV"
        assert bool((ws_buf[need:] == 0x5A).all()), "backward wrote past the workspace size it reported"
        assert _canaries_ok(o_buf, in_o) and _canaries_ok(do_buf, X.inside(do_buf, lambda t: t[:, :Lq, :H, :dh]))
        outs.append(g_buf.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "backward not bitwise reproducible"
    for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
        got = t.double().cpu()
        assert not got.isnan().any(), f"{name}: {int(got.isnan().sum())} elements never written"
        # graded dQ / dK: the product with scale rounds in fp32 first (one ulp)
        exact_model = not (graded and name in ("dQ", "dK"))
        _check(name, got, ref[name.lower()], ref["mag"][name.lower()], dtype, bwd_plan.family, dname, exact_model)


@pytest.mark.parametrize("cid", list(X.CASES))
def test_attention_exact(device, cid):
    run_case(cid, device)
