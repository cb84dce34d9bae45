"""The streamed attention kernels on random data, through functional.attention_core: past 640 keys the 16-bit dh = 64
route is attn_long_* (functional.ATTN_LONG), checked against float64 on the same 16-bit operands and against the generic
kernels the same call took before, under the bounds tests/test_gpu_ops.py holds the resident MFMA kernels to."""
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 1.2e-2, torch.float16: 2e-3}      # test_attention_backward_one_pass_matches_the_kernel_pair's


@pytest.fixture(scope="module")
def dvt():
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _count_calls(monkeypatch, ops):
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.attention_long_fwd, ops.attention_long_bwd

    def cfwd(*a, **kw):
        calls["fwd"] += 1
        return fwd(*a, **kw)

    def cbwd(*a, **kw):
        calls["bwd"] += 1
        return bwd(*a, **kw)

    monkeypatch.setattr(ops, "attention_long_fwd", cfwd)
    monkeypatch.setattr(ops, "attention_long_bwd", cbwd)
    return calls


def _run(F, q, k, v, do, scale):
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = F.attention_core(qd, kd, vd, scale)
    out.backward(do)
    torch.cuda.synchronize()
    return [t.detach().double().cpu() for t in (out, qd.grad, kd.grad, vd.grad)]


def _reference(q, k, v, do, scale):
    q64, k64, v64 = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(q64 @ k64.transpose(-1, -2) * scale, -1) @ v64
    o.backward(do.double().cpu())
    return [o.detach(), q64.grad, k64.grad, v64.grad]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Lq,Lk", [(1, 2, 700, 700), (2, 2, 100, 900), (1, 1, 1569, 1569)])
def test_attention_core_past_640_keys(dvt, device, monkeypatch, dtype, B, H, Lq, Lk):
    F, ops = dvt.functional, dvt.ops
    g = torch.Generator().manual_seed(Lq + Lk)
    dh, scale = 64, 64 ** -0.5
    q = (torch.randn(B, H, Lq, dh, generator=g) * 0.7).to(dtype).cuda()
    k = (torch.randn(B, H, Lk, dh, generator=g) * 0.7).to(dtype).cuda()
    v = (torch.randn(B, H, Lk, dh, generator=g) * 0.7).to(dtype).cuda()
    do = torch.randn(B, Lq, H, dh, generator=g).to(dtype).cuda().permute(0, 2, 1, 3)
    assert ops.attention_plan(q, k, v, q).family == "generic"         # what this call launched before
    calls = _count_calls(monkeypatch, ops)
    assert F.ATTN_LONG is True
    got = _run(F, q, k, v, do, scale)
    assert calls == {"fwd": 1, "bwd": 1}
    monkeypatch.setattr(F, "ATTN_LONG", False)
    generic = _run(F, q, k, v, do, scale)
    assert calls == {"fwd": 1, "bwd": 1}
    ref = _reference(q, k, v, do, scale)
    tol = TOL[dtype]
    for name, a, b, r in zip(("o", "dq", "dk", "dv"), got, generic, ref):
        ea, eb, eab = rel_l2(a, r), rel_l2(b, r), rel_l2(a, b)
        print(f"{name}: streamed {ea:.3e} generic {eb:.3e} streamed vs generic {eab:.3e} (bound {tol:.1e})")
        assert torch.isfinite(a).all()
        assert ea < tol and eb < tol and eab < tol, name


def test_short_sequences_and_single_queries_keep_their_kernels(dvt, device, monkeypatch):
    """up to 640 keys, and one query per (b, h) at any length, the call is today's"""
    F, ops = dvt.functional, dvt.ops
    calls = _count_calls(monkeypatch, ops)
    g = torch.Generator().manual_seed(5)
    for Lq, Lk in ((640, 640), (1, 900)):
        q = torch.randn(1, 2, Lq, 64, generator=g).to(torch.bfloat16).cuda()
        k = torch.randn(1, 2, Lk, 64, generator=g).to(torch.bfloat16).cuda()
        do = torch.randn(1, Lq, 2, 64, generator=g).to(torch.bfloat16).cuda().permute(0, 2, 1, 3)
        got = _run(F, q, k, k, do, 0.125)
        ref = _reference(q, k, k, do, 0.125)
        assert rel_l2(got[0], ref[0]) < TOL[torch.bfloat16]
    assert calls == {"fwd": 0, "bwd": 0}


def test_attention_softmax_spike_in_the_last_chunk(dvt, device):
    """the online-softmax rescale across a chunk seam: one key in the last of three chunks dominates a row whose running
    maximum the first two chunks set"""
    F, ops = dvt.functional, dvt.ops
    g = torch.Generator().manual_seed(10)
    dh = 64
    z = torch.zeros(1, 1, 700, dh, dtype=torch.bfloat16)
    chunk = ops.attention_long_plan(z, z, z, z).k_chunk
    # three chunks exactly (the entry point itself), and the last chunk of a sequence functional routes to these kernels
    for L, direct in ((2 * chunk + 40, True), (max(2 * chunk + 40, 700), False)):
        nch = -(-L // chunk)
        assert nch >= 3
        q = torch.randn(1, 1, L, dh, generator=g)
        k = torch.randn(1, 1, L, dh, generator=g)
        v = torch.randn(1, 1, L, dh, generator=g)
        spike = (nch - 1) * chunk + 7
        k[0, 0, spike] = 6.0 * q[0, 0, 3]
        qb, kb, vb = (t.to(torch.bfloat16) for t in (q, k, v))
        p = torch.softmax(qb.double() @ kb.double().transpose(-1, -2) * dh ** -0.5, -1)
        assert float(p[0, 0, 3, spike]) > 0.99
        ref = p @ vb.double()
        if direct:
            out = torch.empty(1, L, 1, dh, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3)
            ops.attention_long_fwd(qb.cuda(), kb.cuda(), vb.cuda(), out, dh ** -0.5)
        else:
            assert L > 640
            out = F.attention_core(qb.cuda(), kb.cuda(), vb.cuda(), dh ** -0.5)
        assert torch.isfinite(out).all()
        assert rel_l2(out.double().cpu(), ref) < 1e-2
        assert rel_l2(out[0, 0, 3].double().cpu(), ref[0, 0, 3]) < 1e-2
