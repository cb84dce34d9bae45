"""CPU gate on the attention family's exact tests: every attention.hip kernel symbol of the built library is launched by a
named case of tests/test_gpu_attention_exact.py -- the library's own plan query (dvt_attention_plan) says that case takes
that instantiation -- or listed as unreachable with a reason; and the operands of those cases are exact and see a
dropped key, a dropped 32-key step, a missing key mask, swapped heads and a shifted query row."""
import os
import re

import pytest
import torch

from tests import attn_exact as X

# attention.hip kernel symbols that no descriptor reaches, with the reason
UNREACHABLE = {}


def _case_symbols():
    """{kernel symbol: first case id (of test_attention_exact) whose plans launch it}"""
    out = {}
    for cid in X.CASES:
        fwd, bwd = X.plans(cid)
        for sym in X.plan_symbols(fwd, bwd, X.CASES[cid]["dtype"]):
            out.setdefault(sym, f"test_attention_exact[{cid}]")
    return out


def _built_symbols():
    from tools.isa_listing import kernel_listings
    import dvt_amd
    lib = os.path.join(os.path.dirname(dvt_amd.__file__), "libdvt_hip.so")
    names = kernel_listings(lib, demangle=True)
    pat = re.compile(r"^void \(anonymous namespace\)::(attn_(?:fwd|bwd|small|delta)\w*<[^()]*>)\(")
    return {m.group(1) for n in names for m in [pat.match(n)] if m}


def test_every_attention_kernel_is_launched_by_a_case():
    built = _built_symbols()
    assert len(built) == 108, f"attention.hip builds {len(built)} kernels; update the gate"
    launched = _case_symbols()
    missing = sorted(s for s in built if s not in launched and s not in UNREACHABLE)
    assert not missing, f"attention kernels no exact case launches: {missing}"
    stale = sorted(s for s in launched if s not in built)
    assert not stale, f"cases plan kernels the library does not build: {stale}"


def _store_modes(plan, dname):
    """{(kernel symbol, whole-row patch stores?)} of the launches of a plan that have the choice"""
    if plan.family in ("res", "online"):
        return {(X.fwd_symbols(plan, dname)[0], plan.patch)}
    if plan.family == "pair":
        dq, dkv = X.bwd_symbols(plan, dname)
        return {(dq, plan.patch), (dkv, plan.patch2)}
    return set()


def _reachable_store_modes(dname):
    """every (instantiation, store mode) the launchers can take for dh = 64: all (16-query tiles, padded length) pairs of
    both sides, i.e. lengths 16 t + 1 up to 640, forward, one-pass and two-pass backward"""
    from dvt_amd import ops
    dt = X.TORCH_DTYPES[dname]
    buf = torch.zeros(1, 641, 3, 1, 64, dtype=dt)
    lens = list(range(1, 641, 16)) + [640]
    out = set()
    for Lq in lens:
        for Lk in lens:
            q = buf[:, :Lq, 0].permute(0, 2, 1, 3)
            k = buf[:, :Lk, 1].permute(0, 2, 1, 3)
            v = buf[:, :Lk, 2].permute(0, 2, 1, 3)
            o = q
            out |= _store_modes(ops.attention_plan(q, k, v, o), dname)
            out |= _store_modes(ops.attention_plan(q, k, v, o, bwd=True, two_pass=True), dname)
    return out


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
def test_every_store_mode_is_launched_by_a_case(dname):
    """each instantiation with a choice of store mode (whole rows through LDS patches / per lane) runs in every mode the
    launchers can give it"""
    want = _reachable_store_modes(dname)
    got = set()
    for cid, c in X.CASES.items():
        if c["dtype"] == dname:
            for p in X.plans(cid):
                got |= _store_modes(p, dname)
    missing = sorted(want - got)
    assert not missing, f"(kernel, patch stores) pairs no case launches: {missing}"
    assert any(m for _, m in want) and any(not m for _, m in want)


def test_case_plans():
    """the families and counts the cases are there to reach"""
    seen = set()
    for cid, c in X.CASES.items():
        fwd, bwd = X.plans(cid)
        d = c["dtype"]
        seen.add((d, "fwd", fwd.family, fwd.count))
        seen.add((d, "bwd", bwd.family, bwd.count))
        if bwd.family == "pair":
            seen.add((d, "dkv", bwd.count2))
        assert bwd.workspace == (bwd.family in ("pair", "generic"))
        if c["Lk"] == 640:
            assert fwd.family == "online"
    for d in ("bf16", "fp16"):
        for n in range(1, 12):
            assert (d, "fwd", "res", n) in seen, (d, "res", n)
        for n in range(1, 8):
            assert (d, "bwd", "fused", n) in seen, (d, "fused", n)
        for n in range(0, 12):
            assert (d, "bwd", "pair", n) in seen, (d, "dq", n)
            assert (d, "dkv", n) in seen, (d, "dkv", n)
        assert (d, "fwd", "online", 0) in seen and (d, "fwd", "q1", 0) in seen


def test_plan_follows_the_scale_and_refuses_what_the_launcher_refuses():
    from dvt_amd import ops
    buf = torch.zeros(1, 1, 64, 64, dtype=torch.bfloat16)
    assert ops.attention_plan(buf, buf, buf, buf).family == "res"
    assert ops.attention_plan(buf, buf, buf, buf, scale=-0.125).family == "generic"     # mfma kernels need scale > 0
    q = torch.zeros(1, 1, 1, 600).expand(1, 1, 8, 600)          # (zero row strides: only the shapes matter here)
    k = torch.zeros(1, 1, 1, 600).expand(1, 1, 40000, 600)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.attention_plan(q, k, k, q)


def test_graded_scale_makes_c2_one():
    assert X.graded_scale_ok()


def _ops(cid):
    c = X.CASES[cid]
    return X.operands(c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["mode"], X.seed_of(cid)), c


def _ref(ops4, c, **kw):
    return X.reference(*ops4, X.scale_of(c["mode"]), graded=c["mode"] == "graded", **kw)


def _differs(a, b, dtype):
    """some output moves by more than one ulp of dtype (dK / dV where both have the same keys)"""
    names = ("o", "dq", "dk", "dv") if a["dk"].shape == b["dk"].shape else ("o", "dq")
    return any(bool(((a[n] - b[n]).abs() > X.ulp(a[n], dtype)).any()) for n in names)


def _keys_seen(r, v, dtype):
    """per key j (of each (b, h)): does dropping it move some O row by more than one ulp of dtype?  Exact in float64: a row
    with probability p on j is O = (1 - p) O' + p V_j, so without j it is O' = (O - p V_j) / (1 - p); a row whose only key
    it is (p == 1) loses every key it selects."""
    p, o = r["p"], r["o"]
    BH = p.shape[0] * p.shape[1]
    p, o, v = p.reshape(BH, *p.shape[2:]), o.reshape(BH, *o.shape[2:]), v.reshape(BH, *v.shape[2:])
    ul = X.ulp(o, dtype)
    seen = torch.zeros(BH, p.shape[2], dtype=torch.bool)
    for j0 in range(0, p.shape[2], 32):
        pj = p[:, :, j0:j0 + 32, None]                              # [BH, Lq, 32, 1]
        vj = v[:, None, j0:j0 + 32, :]                              # [BH, 1, 32, dh]
        part = (pj > 0) & (pj < 1)
        o2 = (o[:, :, None] - pj * vj) / torch.where(part, 1 - pj, torch.ones_like(pj))
        moved = ((o2 - o[:, :, None]).abs() > ul[:, :, None]).any(-1) & part[..., 0]
        seen[:, j0:j0 + 32] = (moved | (pj[..., 0] == 1)).any(1)
    return seen


CIDS_16 = [cid for cid, c in X.CASES.items() if c["dtype"] != "fp32"]
CIDS_32 = [cid for cid, c in X.CASES.items() if c["dtype"] == "fp32"]


@pytest.mark.parametrize("cid", CIDS_16 + CIDS_32)
def test_operands_are_exact(cid):
    """what the builder guarantees: small integer operands exact in the type; O, dV and delta representable in it; dS
    representable in bf16 and fp16, and in tied mode dQ and dK too; each key of every (b, h) carries probability in some
    row; each (b, h) draws its own operands"""
    (q, k, v, do), c = _ops(cid)
    dt = X.TORCH_DTYPES[c["dtype"]]
    for t in (q, k, v, do):
        assert X.representable(t, dt)
    r = _ref((q, k, v, do), c)
    assert bool(torch.isfinite(r["o"]).all())
    for n in ("o", "dv", "delta"):
        assert X.representable(r[n], dt), n
    for d16 in (torch.bfloat16, torch.float16):    # the MFMA backward rounds dS to 16 bits
        assert X.representable(r["ds"], d16), ("dS", d16)
        if c["mode"] == "tied":                     # scale 1/8: dQ and dK exact too (graded: one fp32 rounding of scale)
            assert X.representable(r["dq"], d16) and X.representable(r["dk"], d16), ("dQ / dK", d16)
    if c["mode"] == "tied":       # probabilities exactly 0 or 1/n, n a power of two
        p = r["p"]
        nz = p[p > 0]
        inv = 1.0 / nz
        assert torch.equal(inv, torch.exp2(torch.round(torch.log2(inv))))
    else:
        mx = (q @ k.transpose(-1, -2)).amax(-1)
        assert c["Lq"] == 1 or (float(mx.max()) > 130 and float(mx.min()) < 10)
    assert bool((r["p"].amax(2) > 0).all()), "a key without probability in any row"
    flat = q.reshape(-1, c["Lq"], c["dh"])
    for i in range(1, flat.shape[0]):
        assert not torch.equal(flat[0], flat[i])


@pytest.mark.parametrize("cid", CIDS_16 + CIDS_32)
def test_operands_see_kernel_errors(cid):
    """the expected outputs move by more than one ulp of the case's type with any single key dropped (every key of every
    (b, h)), any 32-key step dropped, key Lk admitted by the mask, two heads swapped, one query row shifted"""
    (q, k, v, do), c = _ops(cid)
    dt = X.TORCH_DTYPES[c["dtype"]]
    base = _ref((q, k, v, do), c)
    Lk, Lq = c["Lk"], c["Lq"]
    seen = _keys_seen(base, v, dt)
    assert bool(seen.all()), f"keys whose loss no O row shows: {(~seen).nonzero()[:8].tolist()}"
    for s0 in range(0, Lk, 32):
        keep = [i for i in range(Lk) if not s0 <= i < s0 + 32]
        if keep:
            assert _differs(base, _ref((q, k[:, :, keep], v[:, :, keep], do), c), dt), f"keys {s0}.. dropped"
    if Lk % 32:
        assert _differs(base, _ref((q, k, v, do), c, Lk_admit=1), dt), "key Lk admitted"
    if c["H"] > 1:
        sw = lambda t: t[:, [1, 0] + list(range(2, c["H"]))]
        assert _differs(base, _ref(tuple(sw(t) for t in (q, k, v, do)), c), dt), "heads swapped"
    if Lq > 1:
        sh = torch.cat([q[:, :, 1:2], q[:, :, 1:]], 2)     # row 0 reads row 1
        assert _differs(base, _ref((sh, k, v, do), c), dt), "query row shifted"
