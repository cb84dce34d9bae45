"""CPU gate on the exact tests of the streamed attention kernels (tests/test_gpu_attention_long_exact.py): the operands of
every case are exact and see the kernel errors they are there to see; every built attn_long_* kernel is launched by a case;
with the blocks and chunks dvt_attention_long_plan reports, each of the three launches has a case at every boundary of its
chunk and its block; the entry points refuse what they do not compute; the resident launchers' decisions are untouched."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from tests import attn_exact as X
from tests import attn_long_exact as XL

ENTRY_POINTS = ("dvt_attention_long_supported", "dvt_attention_long_bwd_workspace_bytes", "dvt_attention_long_fwd",
                "dvt_attention_long_bwd", "dvt_attention_long_plan")


@pytest.fixture(autouse=True, scope="module")
def streamed_entry_points():
    """everything below gates the exact tests of kernels that the header declares and the library exports"""
    import dvt_amd
    lib = dvt_amd._lib.load()
    for name in ENTRY_POINTS:
        assert name in dvt_amd._lib.SIGNATURES and hasattr(lib, name), name
    assert dvt_amd._lib.ABI_VERSION == 5                 # additions only: no struct changed


# ------------------------------------------------------------------ operands
def _ref(ops4, c, **kw):
    return X.reference(*ops4, X.scale_of(c["mode"]), graded=c["mode"] == "graded", **kw)


def _differs(a, b, dtype):
    """some output moves by more than one ulp of dtype (dK / dV where both have the same keys)"""
    names = ("o", "dq", "dk", "dv") if a["dk"].shape == b["dk"].shape else ("o", "dq")
    return any(bool(((a[n] - b[n]).abs() > X.ulp(a[n], dtype)).any()) for n in names)


def _keys_seen(r, v, dtype):
    """per key j of each (b, h): does dropping it move some O row by more than one ulp of dtype?  In float64 a row with
    probability p on j is O = (1 - p) O' + p V_j, so without j it is O' = (O - p V_j) / (1 - p); a row whose only key it is
    (p == 1) loses every key it selects."""
    p, o = r["p"], r["o"]
    BH = p.shape[0] * p.shape[1]
    p, o, v = p.reshape(BH, *p.shape[2:]), o.reshape(BH, *o.shape[2:]), v.reshape(BH, *v.shape[2:])
    ul = X.ulp(o, dtype)
    seen = torch.zeros(BH, p.shape[2], dtype=torch.bool)
    for j0 in range(0, p.shape[2], 32):
        pj = p[:, :, j0:j0 + 32, None]
        vj = v[:, None, j0:j0 + 32, :]
        part = (pj > 0) & (pj < 1)
        o2 = (o[:, :, None] - pj * vj) / torch.where(part, 1 - pj, torch.ones_like(pj))
        moved = ((o2 - o[:, :, None]).abs() > ul[:, :, None]).any(-1) & part[..., 0]
        seen[:, j0:j0 + 32] = (moved | (pj[..., 0] == 1)).any(1)
    return seen


@pytest.mark.parametrize("cid", list(XL.CASES))
def test_operands_are_exact(cid):
    """small integer operands exact in the type; O, dV and delta representable in it; dS representable in bf16 and fp16, and
    in tied mode dQ and dK too; each key of every (b, h) carries probability in some row; each (b, h) its own draw"""
    c = XL.CASES[cid]
    (q, k, v, do), r = XL.operands_and_reference(cid)
    dt = X.TORCH_DTYPES[c["dtype"]]
    for t in (q, k, v, do):
        assert X.representable(t, dt)
    assert bool(torch.isfinite(r["o"]).all())
    for n in ("o", "dv", "delta"):
        assert X.representable(r[n], dt), n
    for d16 in (torch.bfloat16, torch.float16):
        assert X.representable(r["ds"], d16), ("dS", d16)
        if c["mode"] == "tied":
            assert X.representable(r["dq"], d16) and X.representable(r["dk"], d16), ("dQ / dK", d16)
    if c["mode"] == "tied":                              # probabilities exactly 0 or 1/n, n a power of two
        nz = r["p"][r["p"] > 0]
        inv = 1.0 / nz
        assert torch.equal(inv, torch.exp2(torch.round(torch.log2(inv))))
    else:
        mx = (q @ k.transpose(-1, -2)).amax(-1)
        assert float(mx.max()) > 130 and float(mx.min()) < 10
    assert bool((r["p"].amax(2) > 0).all()), "a key without probability in any row"
    flat = q.reshape(-1, c["Lq"], c["dh"])
    for i in range(1, flat.shape[0]):
        assert not torch.equal(flat[0], flat[i])


@functools.lru_cache(maxsize=None)
def _perturbed(base):
    """[(what, outputs of the float64 reference under that kernel error)] of a geometry, computed once for both types"""
    c = XL.CASES[base + "-bf16"]
    (q, k, v, do), _ = XL.operands_and_reference(base + "-bf16")
    Lk = c["Lk"]
    keep4 = lambda r: {n: r[n] for n in ("o", "dq", "dk", "dv")}
    out = []
    for s0 in range(0, Lk, 32):
        keep = [i for i in range(Lk) if not s0 <= i < s0 + 32]
        if keep:
            out.append((f"keys {s0}.. dropped", keep4(_ref((q, k[:, :, keep], v[:, :, keep], do), c))))
    if Lk % 32:
        out.append(("key Lk admitted", keep4(_ref((q, k, v, do), c, Lk_admit=1))))
    if c["H"] > 1:
        sw = lambda t: t[:, [1, 0] + list(range(2, c["H"]))]
        out.append(("heads swapped", keep4(_ref(tuple(sw(t) for t in (q, k, v, do)), c))))
    sh = torch.cat([q[:, :, 1:2], q[:, :, 1:]], 2)       # row 0 reads row 1
    out.append(("query row shifted", keep4(_ref((sh, k, v, do), c))))
    return out


@pytest.mark.parametrize("cid", list(XL.CASES))
def test_operands_see_kernel_errors(cid):
    """the expected outputs move by more than one ulp of the case's type with any single key dropped (every key of every
    (b, h)), any 32-key step dropped, key Lk admitted by the mask, two heads swapped, one query row shifted"""
    c = XL.CASES[cid]
    (q, k, v, do), base = XL.operands_and_reference(cid)
    dt = X.TORCH_DTYPES[c["dtype"]]
    seen = _keys_seen(base, v, dt)
    assert bool(seen.all()), f"keys whose loss no O row shows: {(~seen).nonzero()[:8].tolist()}"
    for what, r in _perturbed(cid.rsplit("-", 1)[0]):
        assert _differs(base, r, dt), what


# ------------------------------------------------------------------ kernels and boundaries
def _built_symbols():
    from tools.isa_listing import kernel_listings
    import dvt_amd
    lib = os.path.join(os.path.dirname(dvt_amd.__file__), "libdvt_hip.so")
    names = kernel_listings(lib, demangle=True)
    pat = re.compile(r"^void \(anonymous namespace\)::(attn_long_\w*<[^()]*>)\(")
    return {m.group(1) for n in names for m in [pat.match(n)] if m}


def test_every_streamed_kernel_is_launched_by_a_case():
    built = _built_symbols()
    assert len(built) == 6, f"attention.hip builds {len(built)} attn_long_* kernels; update the gate"
    launched = {}
    for cid, c in XL.CASES.items():
        fwd, bwd = XL.plans(cid)                          # (raises if the entry points refuse the case)
        assert fwd.grid > 0 and bwd.grid > 0 and bwd.grid2 > 0 and bwd.workspace
        f, b = XL.symbols(c["dtype"])
        for sym in f + b:
            launched.setdefault(sym, cid)
    assert sorted(launched) == sorted(built)


def _sides(cid):
    """per launch of a case: (rows of the register side, its block, rows of the streamed side, its chunk, patch stores)"""
    c = XL.CASES[cid]
    fwd, bwd = XL.plans(cid)
    return {"fwd": (c["Lq"], fwd.q_block, c["Lk"], fwd.k_chunk, fwd.patch),
            "dq": (c["Lq"], bwd.q_block, c["Lk"], bwd.k_chunk, bwd.patch),
            "dkv": (c["Lk"], bwd.k_block, c["Lq"], bwd.q_chunk, bwd.patch2)}


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("launch", ["fwd", "dq", "dkv"])
def test_cases_cover_the_boundaries_of_every_launch(launch, dname):
    sides = [_sides(cid)[launch] for cid, c in XL.CASES.items() if c["dtype"] == dname]
    for _, blk, _, chunk, _ in sides:
        assert chunk % 32 == 0 and blk % 16 == 0
    assert any(n % chunk == 1 and n > chunk for _, _, n, chunk, _ in sides), "one element in the last chunk"
    assert any(n % chunk == 0 for _, _, n, chunk, _ in sides), "an exact multiple of the chunk"
    assert any(n > 2 * chunk for _, _, n, chunk, _ in sides), "at least three chunks"
    assert any(n < chunk for _, _, n, chunk, _ in sides), "less than one chunk"
    assert any(m < 16 for m, _, _, _, _ in sides), "a register side shorter than a tile"
    assert any(m > blk and m % blk for m, blk, _, _, _ in sides), "two blocks, the last one ragged"
    assert any(m % blk == 0 for m, blk, _, _, _ in sides), "whole blocks"
    # the plan has no choice of store mode: every launch stores whole rows through LDS patches
    assert {patch for *_, patch in sides} == {True}


def test_plan_reports_the_geometry():
    from dvt_amd import ops
    buf = torch.zeros(2, 3137, 3, 3, 64, dtype=torch.bfloat16)
    q, k, v = (buf[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    f = ops.attention_long_plan(q, k, v, q)
    b = ops.attention_long_plan(q, k, v, q, bwd=True)
    assert f.grid == 2 * 3 * -(-3137 // f.q_block) and f.chunks == -(-3137 // f.k_chunk) and f.ring >= 2
    assert f.k_block == 0 and f.patch2 is None and not f.workspace
    assert b.grid2 == 2 * 3 * -(-3137 // b.k_block) and b.chunks2 == -(-3137 // b.q_chunk) and b.ring2 >= 2
    assert (f.q_block, f.k_chunk, f.waves, f.lds) == (b.q_block, b.k_chunk, b.waves, b.lds)
    assert f.q_block == 16 * f.waves and b.k_block == 16 * b.waves2          # one 16-row tile per wave
    for lds, ring, chunk in ((f.lds, f.ring, f.k_chunk), (b.lds2, b.ring2, b.q_chunk)):
        assert ring * 2 * chunk * 128 <= lds <= 80 * 1024                     # two workgroups per CU


# ------------------------------------------------------------------ refusals
def _views(dtype=torch.bfloat16, dh=64, skew=False, L=700):
    dhb = dh + 1 if skew else dh
    buf = torch.zeros(1, L, 3, 2, dhb, dtype=dtype)
    return [buf[:, :, i, :, :dh].permute(0, 2, 1, 3) for i in range(3)]


REFUSED = {
    "fp32": dict(dtype=torch.float32),
    "dh32": dict(dh=32),
    "dropout": dict(dropout_p=0.1),
    "skew": dict(skew=True),
    "negative_scale": dict(scale=-0.125),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_entry_points_refuse(what):
    from dvt_amd import ops
    import dvt_amd
    L = dvt_amd._lib
    kw = dict(REFUSED[what])
    dropout_p, scale = kw.pop("dropout_p", 0.0), kw.pop("scale", None)
    q, k, v = _views(**kw)
    assert not ops.attention_long_supported(q, k, v, q, scale=scale, dropout_p=dropout_p)
    assert not ops.attention_long_supported(q, k, v, q, scale=scale, dropout_p=dropout_p, do=q)
    for bwd in (False, True):
        with pytest.raises(RuntimeError, match="status -2"):
            ops.attention_long_plan(q, k, v, q, bwd=bwd, scale=scale, dropout_p=dropout_p)
    # the launchers themselves: refused on the host, before any launch
    lse = torch.zeros(1, 2, 700)
    d = ops._attn_desc(q, k, v, q, lse, q.shape[3] ** -0.5 if scale is None else scale)
    d.d_o, d.dq, d.dk, d.dv = q.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.workspace = lse.data_ptr()
    if dropout_p:
        d.dropout_p, d.rng_state = dropout_p, 256
    lib = L.load()
    unsupported = L.ENUMS["dvt_status"]["DVT_ERR_UNSUPPORTED"]
    assert lib.dvt_attention_long_fwd(C.byref(d), None) == unsupported
    assert lib.dvt_attention_long_bwd(C.byref(d), None) == unsupported
    assert lib.dvt_attention_long_supported(C.byref(d), 0) == 0 and lib.dvt_attention_long_supported(C.byref(d), 1) == 0


def test_supported_views_and_misaligned_gradients():
    from dvt_amd import ops
    q, k, v = _views()
    assert ops.attention_long_supported(q, k, v, q) and ops.attention_long_supported(q, k, v, q, do=q)
    off = torch.zeros(700 * 2 * 64 + 4, dtype=torch.bfloat16)[4:].view(1, 700, 2, 64).permute(0, 2, 1, 3)   # 8-byte aligned
    assert not ops.attention_long_supported(off, k, v, q)
    assert ops.attention_long_supported(q, k, v, q, do=q, dq=q) and not ops.attention_long_supported(q, k, v, q, do=q, dk=off)


def test_resident_launchers_keep_their_decisions():
    """gen_k700's views still take the generic kernels through dvt_attention_fwd / _bwd"""
    fwd, bwd = X.plans("gen_k700-bf16")
    assert fwd.family == "generic" and bwd.family == "generic"
    fwd, bwd = X.plans("gen_k700-fp16")
    assert fwd.family == "generic" and bwd.family == "generic"
