#!/usr/bin/env python3
"""Find MFMAs that accumulate onto the result of an MFMA of ANOTHER shape too soon after it, in the gfx950 listing.

The hazard (profiles/r06_mfma_shape_hazard.md).  The hardware interlocks a dependent accumulate -- SrcC of an MFMA overlapping
the vDst of an earlier one -- only when the two have the same opcode and the same registers.  hipcc 7.2's hazard recognizer
also treats "SrcC is exactly the earlier vDst" with DIFFERENT opcodes as that case and emits no wait states, so a
v_mfma_f32_16x16x16_* right behind a v_mfma_f32_16x16x32_* on one accumulator (or the reverse) reads part of it stale: no
error, a k-step missing from the sum.  Round 5's window forward (conv3x1_fwd_kernel at one position block per wave) lost
exactly one 16x16x32 step that way.

The rule.  A pair (writer W, reader R) -- R's SrcC overlaps W's vDst, VGPR ranges v[a:b] or AGPR ranges a[a:b] -- is a
candidate when the opcodes differ (exact or partial overlap) or the opcodes match but the overlap is partial.  A candidate
is safe on a path when, strictly between W and R on that path, there are
    at least MIN_MFMAS (3) other MFMAs, or at least MIN_STATES (16) wait states
(`s_nop N` counts N + 1, every other instruction 1).  Where the margin comes from:
  * 16 states are the fence that fixed round 5 (`mfma_shape_fence`, csrc/conv3x1_fwd.hip: `s_nop 15` = 64 cycles, past
    the 16-cycle issue + write-back of either shape);
  * the round-5 table: with the fence removed (-DDVT_NO_MFMA_SHAPE_FENCE) the window forward put 0 / 1 / 2 MFMAs between
    the shapes at 1 / 2 / 3 position blocks per wave and 3 or more from 4 blocks up; 1 block failed on the GPU, 2 and 3 did
    not fail on the data tried -- which is not evidence of safety, so they stay below the margin -- and 4 - 6 passed.
    Three independent 16x16x32 / 16x16x16 MFMAs hold the vector issue for at least 3 x 8 cycles plus their own pipeline.
A pair must be safe on EVERY path: the distance is the minimum over the control-flow graph, back edges included (the
tap loops: a tap's 16x16x16 tail feeds the next tap's first 16x16x32 step across the loop edge).  The listing is cut into
basic blocks at branch targets and after s_branch / s_cbranch_* / s_setpc / s_endpgm (a branch's simm16 is sign-extended:
the listing prints it unsigned; a target that is not an instruction of the kernel is an error); a forward dataflow carries, per
in-flight MFMA result, the Pareto-minimal (wait states, MFMAs) since it was written on any path reaching the block, to a
fixed point.  Later MFMAs that overwrite a register end its dependence on the earlier writer (only the nearest writer of
a register on a path is its producer).  Distances at or past HORIZON states are not tracked.

Out of scope: other hazard classes (VALU -> MFMA operands, MFMA -> VALU reads) and wait states inside inline-asm strings.

usage: tools/check_mfma_hazards.py [path/to/libdvt_hip.so or csrc object]     (exit 1 on any pair below the margin; prints
                                                                                every kernel that mixes MFMA opcodes on one
                                                                                accumulator with its minimum distances)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_listing import kernel_listings  # noqa: E402

MIN_MFMAS = 3
MIN_STATES = 16
HORIZON = 64
# Kernel-name substrings whose flagged pairs are known safe, each with the committed measurement that shows it.  Empty:
# every flagged site is fenced in the source instead.
ALLOWED = {}

_REG = re.compile(r"^([va])(?:\[(\d+):(\d+)\]|(\d+))$")
_BRANCH = re.compile(r"^s_(branch|cbranch_\w+)\s+(-?\d+)")


def _regs(op):
    """register set of one operand (VGPRs as v indices, AGPRs offset by 1024), empty for a constant"""
    m = _REG.match(op)
    if not m:
        return frozenset()
    lo = int(m.group(2) if m.group(2) is not None else m.group(4))
    hi = int(m.group(3)) if m.group(3) is not None else lo
    base = 1024 if m.group(1) == "a" else 0
    return frozenset(range(base + lo, base + hi + 1))


def _weight(text):
    m = re.match(r"s_nop\s+(\d+)", text)
    return int(m.group(1)) + 1 if m else 1


def _mfma(text):
    """(opcode, vDst registers, SrcC registers) of an MFMA instruction, else None"""
    if not text.startswith("v_mfma"):
        return None
    op, _, rest = text.partition(" ")
    ops = [o.strip() for o in rest.split(",")]
    # v_mfma D, A, B, C [modifiers]: the ranges themselves contain no comma
    return op, _regs(ops[0]), _regs(ops[3].split()[0])


def _blocks(insns):
    """basic blocks of a listing: [(first, last_excl)], successor lists"""
    n = len(insns)
    index = {a: i for i, (a, _) in enumerate(insns)}
    leaders = {0}
    succ_of = {}
    for i, (a, t) in enumerate(insns):
        m = _BRANCH.match(t)
        if m:
            # SOPP simm16, in dwords from the next instruction; llvm-objdump prints it unsigned (a backward branch is 65532)
            off = int(m.group(2))
            if off >= 0x8000:
                off -= 0x10000
            tgt = index.get(a + 4 + 4 * off)
            if tgt is None:
                raise ValueError(f"branch at {a:#x} ({t}) targets {a + 4 + 4 * off:#x}, not an instruction of the kernel")
            s = [tgt]
            if m.group(1) != "branch" and i + 1 < n:
                s.append(i + 1)
            succ_of[i] = s
            leaders.update(s)
            if i + 1 < n:
                leaders.add(i + 1)
        elif t.startswith(("s_endpgm", "s_setpc_b64", "s_trap")):
            succ_of[i] = []
            if i + 1 < n:
                leaders.add(i + 1)
    starts = sorted(leaders)
    blocks = [(s, starts[k + 1] if k + 1 < len(starts) else n) for k, s in enumerate(starts)]
    bid = {s: k for k, (s, _) in enumerate(blocks)}
    succ = []
    for s, e in blocks:
        last = e - 1
        nxt = succ_of.get(last, [e] if e < n else [])
        succ.append([bid[x] for x in nxt if x in bid])
    return blocks, succ


def back_edges(insns):
    """number of CFG edges of a listing that go to a block at or before their own (the loops)"""
    blocks, succ = _blocks(insns)
    return sum(1 for b, ss in enumerate(succ) for x in ss if x <= b)


def _add(facts, key, d):
    """insert distance d = (states, mfmas) into the Pareto set facts[key]; -> whether it changed"""
    cur = facts.get(key, ())
    if any(c[0] <= d[0] and c[1] <= d[1] for c in cur):
        return False
    facts[key] = tuple(c for c in cur if not (d[0] <= c[0] and d[1] <= c[1])) + (d,)
    return True


def _walk(insns, dec, s, e, facts_in, pairs):
    """run block [s, e) from facts_in {(writer, regs): ((states, mfmas), ..)}; record reads into pairs; -> facts out"""
    live = [(w, regs, d) for (w, regs), ds in facts_in.items() for d in ds]    # d: distance at the block's start
    S = M = 0                                                                   # states / MFMAs passed inside the block
    for i in range(s, e):
        mf = dec[i]
        if mf is not None:
            op, dst, src = mf
            if src:
                for w, regs, d in live:
                    if regs & src and d[0] + S < HORIZON:
                        pairs.setdefault((w, i), set()).add((d[0] + S, d[1] + M))
            S += 1
            M += 1
            nl = []
            for w, regs, d in live:
                if d[0] + S >= HORIZON:
                    continue
                if regs & dst:
                    regs = regs - dst
                    if not regs:
                        continue
                nl.append((w, regs, d))
            nl.append((i, dst, (-S, -M)))
            live = nl
        else:
            S += _weight(insns[i][1])
    out = {}
    for w, regs, d in live:
        dd = (d[0] + S, d[1] + M)
        if dd[0] < HORIZON:
            _add(out, (w, regs), dd)
    return out


def analyze(insns):
    """-> {(writer index, reader index): {(states, mfmas), ..}} for every MFMA pair with SrcC / vDst overlap within HORIZON"""
    dec = [_mfma(t) for _, t in insns]
    if not any(dec):
        return {}
    blocks, succ = _blocks(insns)
    fin = [dict() for _ in blocks]
    fout = [None] * len(blocks)
    work = list(range(len(blocks)))
    queued = set(work)
    while work:
        b = work.pop(0)
        queued.discard(b)
        out = _walk(insns, dec, *blocks[b], fin[b], {})
        if out == fout[b]:
            continue
        fout[b] = out
        for x in succ[b]:
            changed = False
            for k, ds in out.items():
                for d in ds:
                    changed |= _add(fin[x], k, d)
            if changed and x not in queued:
                work.append(x)
                queued.add(x)
    pairs = {}
    for b, (s, e) in enumerate(blocks):
        _walk(insns, dec, s, e, fin[b], pairs)
    return pairs


def _short(op):
    return op[len("v_mfma_"):] if op.startswith("v_mfma_") else op


def kernel_report(insns):
    """-> (mixing, violations): mixing {(writer opcode, reader opcode): (min states, min MFMAs)} over the candidate pairs;
    violations [(writer address, writer text, reader address, reader text, states, mfmas)]"""
    dec = [_mfma(t) for _, t in insns]
    mixing, bad = {}, []
    for (w, r), ds in sorted(analyze(insns).items()):
        (ow, dw, _), (orr, _, cr) = dec[w], dec[r]
        if ow == orr and dw == cr:
            continue                                         # same opcode, same registers: interlocked
        key = (_short(ow), _short(orr))
        ms, mm = mixing.get(key, (HORIZON, HORIZON))
        mixing[key] = (min(ms, min(d[0] for d in ds)), min(mm, min(d[1] for d in ds)))
        for st, mf in sorted(ds):
            if st < MIN_STATES and mf < MIN_MFMAS:
                bad.append((insns[w][0], insns[w][1], insns[r][0], insns[r][1], st, mf))
                break
    return mixing, bad


def short_name(sym):
    """a demangled kernel symbol without its return type, the anonymous namespace and the parameter list"""
    s = sym.replace("(anonymous namespace)::", "")
    if s.startswith("void "):
        s = s[len("void "):]
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(s[i], 0)
            if depth == 0:
                s = s[:i]
                break
    return s


def scan(path):
    """-> {short kernel name: (mixing, violations)} for every kernel of `path` with a candidate pair"""
    out = {}
    for sym, insns in kernel_listings(path, demangle=True).items():
        mixing, bad = kernel_report(insns)
        if mixing:
            out[short_name(sym)] = (mixing, bad)
    return out


def violations(report):
    """the kernels of a scan() report with pairs below the margin, outside ALLOWED"""
    return {k: bad for k, (_, bad) in report.items() if bad and not any(a in k for a in ALLOWED)}


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "data-efficient-video-transformers_amd", "libdvt_hip.so")
    rep = scan(path)
    bad = violations(rep)
    print(f"{len(rep)} kernels mix MFMA opcodes on one accumulator; {len(bad)} with pairs below the margin "
          f"(>= {MIN_MFMAS} MFMAs or >= {MIN_STATES} wait states between them)")
    for k in sorted(rep):
        mixing, _ = rep[k]
        print(f"  {'VIOLATION' if k in bad else 'ok       '} {k}")
        for (a, b), (st, mf) in sorted(mixing.items()):
            print(f"      {a} -> {b}: min {mf} MFMAs, min {st} wait states" + (" (or more)" if st >= HORIZON else ""))
    for k in sorted(bad):
        print(f"{k}:")
        for wa, wt, ra, rt, st, mf in bad[k]:
            print(f"  {wa:#x} {wt}\n  {ra:#x} {rt}\n      {mf} MFMAs, {st} wait states between them")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
