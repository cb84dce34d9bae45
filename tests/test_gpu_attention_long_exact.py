"""Exact tests of the streamed attention kernels (attn_long_* of csrc/attention.hip) through their own entry points, on
the operands of tests/attn_exact.py whose softmax is exact.

The method of tests/test_gpu_attention_exact.py: the forward and the backward (twice: bitwise reproducible) write O, dQ,
dK, dV as views into NaN-filled buffers whose padding carries canaries; lse and the workspace are canaried past their
end; the rows of the inputs past each sequence hold NaN (a kernel that reads them poisons its sums).  The kernels take
exp2 of integer scores (graded) or produce probabilities 0 / 1/n (tied), as the resident MFMA families do, so every
output equals the float64 reference rounded once to the output type; graded dQ / dK (one fp32 rounding of the product
with scale) are within one ulp."""
import ctypes as C

import pytest
import torch

from tests import attn_exact as X
from tests import attn_long_exact as XL

pytestmark = pytest.mark.gpu

CANARY = -29.0          # exact in every type, never an output of these operands


def _check(name, got, ref, dtype, exact):
    if exact:
        assert X.representable(ref, dtype), f"{name}: reference not representable in {dtype}"
    bad = X.mismatch(got, ref, dtype, True if exact else False, ulps=1)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {list(i)}: "
                             f"got {float(got[i])}, want {float(ref[i])}")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _canaries_ok(buf, inner):
    want = torch.full_like(buf, CANARY)
    return bool(torch.equal(_bits(buf)[~inner], _bits(want)[~inner]))


def run_case(cid, device):
    from dvt_amd import ops
    import dvt_amd
    c = XL.CASES[cid]
    dtype = X.TORCH_DTYPES[c["dtype"]]
    B, H, Lq, Lk, dh, mode = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["mode"]
    graded = mode == "graded"
    scale = X.scale_of(mode)
    (q64, k64, v64, do64), ref = XL.operands_and_reference(cid)

    qkv_buf, (q, k, v) = X.layout(c, dtype, device, fill=CANARY)
    qkv_buf[:, Lq:, 0] = float("nan")                   # rows past each sequence: never to be read
    qkv_buf[:, Lk:, 1:] = float("nan")
    for view, val in ((q, q64), (k, k64), (v, v64)):
        view.copy_(val.to(dtype))
    o_buf, o = X.out_layout(c, dtype, device, fill=CANARY)
    o.fill_(float("nan"))
    do_buf, do = X.out_layout(c, dtype, device, fill=CANARY)
    do_buf[:, Lq:] = float("nan")
    do.copy_(do64.to(dtype))
    n_lse = B * H * Lq
    lse_buf = torch.full((n_lse + 64,), CANARY, dtype=torch.float32, device=device)
    lse_buf[:n_lse] = float("nan")

    fwd_plan, bwd_plan = XL.plans(cid)
    assert ops.attention_long_supported(q, k, v, o, scale=scale)
    assert ops.attention_long_supported(q, k, v, o, scale=scale, do=do)
    assert ops.attention_long_plan(q, k, v, o, scale=scale) == fwd_plan
    assert fwd_plan.grid == B * H * -(-Lq // fwd_plan.q_block) and fwd_plan.chunks == -(-Lk // fwd_plan.k_chunk)

    lse = ops.attention_long_fwd(q, k, v, o, scale, lse=lse_buf[:n_lse])
    torch.cuda.synchronize()
    in_o = X.inside(o_buf, lambda t: t[:, :Lq, :H, :dh])
    assert _canaries_ok(o_buf, in_o), "forward wrote outside O"
    assert torch.equal(_bits(lse_buf[n_lse:]), _bits(torch.full_like(lse_buf[n_lse:], CANARY))), "forward wrote past lse"
    got_o = o.double().cpu()
    assert not got_o.isnan().any(), f"O: {int(got_o.isnan().sum())} elements NaN"
    _check("O", got_o, ref["o"], dtype, True)
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
        assert ops.attention_long_plan(q, k, v, o, bwd=True, do=do, dq=dq, dk=dk, dv=dv, scale=scale) == bwd_plan
        need = lib.dvt_attention_long_bwd_workspace_bytes(C.byref(ops._attn_desc(q, k, v, o, lse, scale)))
        assert need == 4 * n_lse
        ws_buf = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=device)
        ops.attention_long_bwd(q, k, v, o, lse, do, dq, dk, dv, scale, ws=ws_buf[:need])
        torch.cuda.synchronize()
        in_g = X.inside(g_buf, lambda t: t[:, :Lq, 0, :H, :dh]) | X.inside(g_buf, lambda t: t[:, :Lk, 1, :H, :dh]) | \
            X.inside(g_buf, lambda t: t[:, :Lk, 2, :H, :dh])
        assert _canaries_ok(g_buf, in_g), "backward wrote outside dQ / dK / dV"
        assert bool((ws_buf[need:] == 0x5A).all()), "backward wrote past the workspace size it reported"
        assert _canaries_ok(o_buf, in_o), "backward wrote to O"
        outs.append(g_buf.clone())
        if rep == 0:
            delta = ws_buf[:need].view(torch.float32).double().cpu()
            assert torch.equal(delta, ref["delta"].reshape(-1)), "delta in the workspace is not rowsum(dO * O)"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "backward not bitwise reproducible"
    for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
        got = t.double().cpu()
        assert not got.isnan().any(), f"{name}: {int(got.isnan().sum())} elements NaN"
        # graded dQ / dK: the product with scale rounds in fp32 first (one ulp)
        _check(name, got, ref[name.lower()], dtype, not (graded and name in ("dQ", "dK")))


@pytest.mark.parametrize("cid", list(XL.CASES))
def test_attention_long_exact(device, cid):
    run_case(cid, device)
