"""Cases of the exact tests of the streamed attention kernels (attn_long_* of csrc/attention.hip).

The operands, their float64 reference and the layouts are those of tests/attn_exact.py; only the case table, the plan query
(dvt_attention_long_plan) and the kernel symbols are this family's.  Every case runs the packed layout in both 16-bit types
and calls the dvt_attention_long_* entry points directly (tests/test_gpu_attention_long_exact.py); the CPU gate
tests/test_attention_long_coverage.py checks the operands and that the cases cover every chunk / block boundary of the
three launches.
"""
import functools

from tests import attn_exact as X

_16 = ("bf16", "fp16")


def _c(B, H, Lq, Lk, mode="tied"):
    return dict(B=B, H=H, Lq=Lq, Lk=Lk, dh=64, mode=mode, layout="packed", two_pass=False, dtypes=_16)


CASES_BASE = {
    "q40_k641": _c(1, 2, 40, 641),                              # one key past the limit of the resident kernels
    "q40_k672_graded": _c(1, 2, 40, 672, mode="graded"),        # a multiple of 32, no tail
    "L705_graded": _c(1, 2, 705, 705, mode="graded"),
    "q130_k1025": _c(2, 2, 130, 1025),                          # two clips; one key in the last chunk; ragged query block
    "q1300_k40": _c(1, 2, 1300, 40),                            # long query side, short key side
    "L1313_graded": _c(1, 1, 1313, 1313, mode="graded"),
    # the boundaries of the chunk and the block on each side (tests/test_attention_long_coverage.py)
    "L768_graded": _c(1, 2, 768, 768, mode="graded"),           # whole chunks and whole blocks on both sides
    "q257_k150": _c(1, 2, 257, 150),                            # one query in the last chunk of the dk/dv launch
    "q9_k700": _c(1, 2, 9, 700),                                # a query side shorter than a tile
    "q700_k9": _c(1, 2, 700, 9),                                # a key side shorter than a tile
}
CASES = {f"{k}-{d}": dict(v, dtype=d) for k, v in CASES_BASE.items() for d in v["dtypes"]}


def seed_of(cid):
    c = CASES[cid]
    return c["Lq"] * 1013 + c["Lk"] * 37 + (11 if c["mode"] == "graded" else 0)


@functools.lru_cache(maxsize=None)
def _shared(base):
    c = CASES_BASE[base]
    ops4 = X.operands(c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["mode"], seed_of(f"{base}-bf16"))
    ref = X.reference(*ops4, X.scale_of(c["mode"]), graded=c["mode"] == "graded")
    return ops4, ref


def operands_and_reference(cid):
    """((q, k, v, do) float64, reference dict) of a case: built once per geometry and shared (read only) by both types"""
    return _shared(cid.rsplit("-", 1)[0])


def plans(cid, device="cpu"):
    """(forward plan, backward plan) of the case's views (ops.attention_long_plan; no launch)"""
    from dvt_amd import ops
    c = CASES[cid]
    dt = X.TORCH_DTYPES[c["dtype"]]
    _, (q, k, v) = X.layout(c, dt, device, fill=0.0)
    _, o = X.out_layout(c, dt, device, fill=0.0)
    scale = X.scale_of(c["mode"])
    return (ops.attention_long_plan(q, k, v, o, scale=scale),
            ops.attention_long_plan(q, k, v, o, bwd=True, do=o, scale=scale))


_ELEM = {"bf16": "std::bfloat16_t", "fp16": "_Float16"}


def symbols(dname):
    """demangled names (without the namespace and the parameter list) of the kernels a forward and a backward launch"""
    E = _ELEM[dname]
    return [f"attn_long_fwd_kernel<{E}>"], [f"attn_long_bwd_dq_kernel<{E}>", f"attn_long_bwd_dkv_kernel<{E}>"]
