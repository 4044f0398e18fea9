#!/usr/bin/env python3
"""What a kernel does before its first multiply-add: the loads it issues and the waits it takes.

    python tools/prologue_chain.py FILE.hip [SUBSTRING ...]      compile FILE.hip to gfx950 device assembly, report the kernels whose
                                                                 (mangled) symbol contains one of the substrings (none: every kernel)
    python tools/prologue_chain.py --bench                       the seven kernels of the B = 64 f32 decode step
    python tools/prologue_chain.py --asm FILE.s [SUBSTRING ...]  an assembly listing made elsewhere
    python tools/prologue_chain.py --whole ...                   (with any of the above) the walk goes on to s_endpgm

The compiler lays basic blocks out in an order of its own (the attention kernel's final merge stands in front of its page loop), so
the listing is cut into basic blocks and walked along its branches.  The multiply-add that ends the prologue is the first FMA / MFMA
in execution order (a block comes after every block that can run before it; a loop's back edge does not count).  Reported, in that
order, are the blocks that lie on some way from the entry to it: every group of scalar loads (destination <- base + offset; base
`kernarg` = the kernel-argument pointer or a copy of it), every group of vector loads, every s_waitcnt.  A block only some waves
run (wave 0's early K page) is part of that list; the labels tell the blocks apart.

Last come the counts.  A wait is *dependent* when a load of its kind was issued since the previous wait of that kind: one memory
round trip the wave cannot overlap with what follows.  They are counted per way through the blocks; the fewest and the most are
printed (scalar: lgkmcnt behind scalar loads; vector: vmcnt behind vector loads).

--whole reports the kernel to its end instead: over the ways that run from the entry THROUGH the first multiply-add to an s_endpgm
(a workgroup that leaves before it has no operands to wait for), the fewest and the most dependent vector waits, and the number of
vector load instructions that stand behind the first multiply-add in execution order -- requests no earlier result can hide.  A
loop's body counts once (its back edge is not followed).

Only load, wait and branch mnemonics (and the FMA / MFMA that ends the prologue) are matched; register writes are followed only as
far as needed to know which scalar pairs still hold the kernel-argument pointer.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music-generation-emotion-adaptive_amd", "csrc")

SLOAD = re.compile(r"^(s_load_dword(?:x(\d+))?|s_buffer_load_dword(?:x(\d+))?)\s+(\S+),\s*(s\[\d+:\d+\]),\s*(\S+)")
VLOAD = re.compile(r"^((?:global|buffer|flat|scratch)_load_\w+)\s+(\S+?),")
LDSLOAD = re.compile(r"^(ds_read\w*|ds_load\w*)\s")
WAIT = re.compile(r"^s_waitcnt\s+(.*)$")
FMA = re.compile(r"^(v_mfma_\w+|v_smfmac_\w+|v_fma_\w+|v_fmac_\w+|v_pk_fma_\w+|v_mac_\w+|v_dot\w+)\s")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
SYMBOL = re.compile(r"^([A-Za-z_][\w$.]*):")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")
SREG = re.compile(r"s\[(\d+):(\d+)\]|s(\d+)")
# user SGPRs in front of the kernel-argument pointer, in the order the hardware loads them
USER_SGPRS_BEFORE_KERNARG = (("private_segment_buffer", 4), ("dispatch_ptr", 2), ("queue_ptr", 2))


def _flags_from_makefile():
    """The flags of csrc/Makefile's CXXFLAGS that change device code."""
    flags = ["-O3", "-std=c++17"]
    try:
        with open(os.path.join(CSRC, "Makefile")) as f:
            for line in f:
                if line.startswith("CXXFLAGS"):
                    words = line.split(":=", 1)[1].split()
                    flags = [w for w in words if w.startswith(("-O", "-std=", "-D"))]
    except OSError:
        pass
    return flags


def find_hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def compile_to_asm(hip_file, extra=()):
    """Device assembly of one .hip file for gfx950 (no GPU needed)."""
    hipcc = find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = [hipcc] + _flags_from_makefile() + ["--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only", "-S",
                                                  os.path.abspath(hip_file), "-o", out] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(hip_file)))
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
        with open(out) as f:
            return f.read()


def split_kernels(text):
    """{symbol: (body lines, kernarg base sgpr index)} for every kernel of a listing."""
    lines = text.splitlines()
    bodies, cur, name = {}, None, None
    for ln in lines:
        s = ln.strip()
        m = SYMBOL.match(ln)
        if m and not m.group(1).startswith(".L") and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if s.startswith((".Lfunc_end", ".section", ".amdhsa_kernel")):
                bodies[name] = cur
                cur = None
            else:
                cur.append(s.split(";")[0].strip())
    if cur is not None:
        bodies[name] = cur
    kern, have, out = None, {}, {}
    for ln in lines:   # kernel descriptors: where the kernel-argument pointer arrives
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            kern, have = s.split()[1], {}
        elif kern and s.startswith(".amdhsa_user_sgpr_"):
            k, _, v = s[len(".amdhsa_user_sgpr_"):].partition(" ")
            try:
                have[k] = int(v.strip(), 0)
            except ValueError:
                have[k] = 0
        elif kern and s.startswith(".end_amdhsa_kernel"):
            base = sum(n for k, n in USER_SGPRS_BEFORE_KERNARG if have.get(k, 0))
            if kern in bodies:
                out[kern] = (bodies[kern], base)
            kern = None
    if not out:   # a bare listing without descriptors: the pointer is s[0:1]
        out = {k: (v, 0) for k, v in bodies.items()}
    return out


def _regs(tok):
    m = SREG.fullmatch(tok.strip().rstrip(","))
    if not m:
        return None
    if m.group(3) is not None:
        return (int(m.group(3)), int(m.group(3)))
    return (int(m.group(1)), int(m.group(2)))


def basic_blocks(body):
    """[(label or None, [instructions], [successor block indices])] in listing order."""
    blocks, cur, label = [], [], None
    for s in body:
        m = LABEL.match(s)
        if m:
            if cur or label is not None:
                blocks.append([label, cur, None])
            cur, label = [], m.group(1)
            continue
        if not s or s.startswith("."):
            continue
        cur.append(s)
        if BRANCH.match(s) or s.startswith("s_endpgm"):
            blocks.append([label, cur, None])
            cur, label = [], None
    if cur or label is not None:
        blocks.append([label, cur, None])
    index = {b[0]: i for i, b in enumerate(blocks) if b[0]}
    for i, b in enumerate(blocks):
        last = b[1][-1] if b[1] else ""
        m = BRANCH.match(last)
        succ = []
        if m:
            if m.group(2) in index:
                succ.append(index[m.group(2)])
            if m.group(1) != "s_branch" and i + 1 < len(blocks):
                succ.append(i + 1)
        elif not last.startswith("s_endpgm") and i + 1 < len(blocks):
            succ.append(i + 1)
        b[2] = succ
    return [tuple(b) for b in blocks]


def _reach(start, succ):
    seen, todo = set(), list(start)
    while todo:
        n = todo.pop()
        if n not in seen:
            seen.add(n)
            todo += succ[n]
    return seen


def prologue_blocks(blocks):
    """(ordered block indices on a way from the entry to the target, target block, forward edges) -- see the module text."""
    n = len(blocks)
    succ = [list(b[2]) for b in blocks]
    has_fma = [any(FMA.match(s) for s in b[1]) for b in blocks]
    # back edges by depth-first search from the entry
    back, state = set(), {}
    stack = [(0, iter(succ[0]))]
    state[0] = 1
    order = []
    while stack:
        u, it = stack[-1]
        for v in it:
            if state.get(v) == 1:
                back.add((u, v))
            elif v not in state:
                state[v] = 1
                stack.append((v, iter(succ[v])))
                break
        else:
            state[u] = 2
            order.append(u)
            stack.pop()
    fwd = [[v for v in succ[u] if (u, v) not in back] for u in range(n)]
    topo = [u for u in reversed(order)]   # reverse post-order: a topological order of the forward edges
    cands = [i for i in topo if has_fma[i]]
    if not cands:
        return topo, None, fwd
    target = cands[0]
    pred = [[] for _ in range(n)]
    for u in range(n):
        for v in fwd[u]:
            pred[v].append(u)
    to_target = _reach([target], pred)
    return [i for i in topo if i in to_target], target, fwd


def whole_counts(body):
    """--whole: ((fewest, most) dependent vector waits over the ways entry -> first multiply-add -> s_endpgm, vector loads behind the
    first multiply-add, [the vmcnt waits and vector-load groups in execution order as text]); None without a multiply-add."""
    blocks = basic_blocks(body)
    if not blocks:
        return None
    before, target, fwd = prologue_blocks(blocks)
    if target is None:
        return None
    after = _reach([target], fwd)
    # a topological order of the blocks behind the target
    indeg = {i: 0 for i in after}
    for u in after:
        for v in fwd[u]:
            if v in after:
                indeg[v] += 1
    tail = []
    ready = [target]
    while ready:
        u = ready.pop()
        tail.append(u)
        for v in fwd[u]:
            if v in after:
                indeg[v] -= 1
                if indeg[v] == 0:
                    ready.append(v)
    # (back edges are not followed, so the forward edges form a DAG and no block is both in front of and behind the target;
    # the filter keeps the walk free of repeats whatever the layout)
    walk = [i for i in before if i != target and i not in after] + tail
    inset_before = set(before)
    late, trace = 0, []
    per_block = {}
    for i in walk:
        ev, seen_fma = [], i != target
        for s in blocks[i][1]:
            if not seen_fma and FMA.match(s):
                seen_fma = True
                ev.append(("fma",))
                continue
            m = VLOAD.match(s)
            if m:
                ev.append(("vload", m.group(1)))
                if i in after and seen_fma:
                    late += 1
                continue
            m = WAIT.match(s)
            if m and "vmcnt" in m.group(1):
                ev.append(("wait", m.group(1).strip()))
        per_block[i] = ev
    best = {walk[0]: {False: (0, 0)}}
    ends = []
    for i in walk:
        states = best.get(i)
        if not states:
            continue
        out = {}
        for pending, (lo, hi) in states.items():
            for e in per_block[i]:
                if e[0] == "vload":
                    pending = True
                elif e[0] == "wait" and pending:
                    lo, hi, pending = lo + 1, hi + 1, False
            o = out.get(pending)
            out[pending] = (min(lo, o[0]), max(hi, o[1])) if o else (lo, hi)
        last = blocks[i][1][-1] if blocks[i][1] else ""
        if i in after and last.startswith("s_endpgm"):
            ends += list(out.values())
        for v in fwd[i]:
            if (i in after and v in after) or (i not in after and v in inset_before):
                dst = best.setdefault(v, {})
                for pending, (lo, hi) in out.items():
                    o = dst.get(pending)
                    dst[pending] = (min(lo, o[0]), max(hi, o[1])) if o else (lo, hi)
    for i in walk:
        n = 0
        for e in per_block[i] + [("end",)]:
            if e[0] == "vload":
                n += 1
                continue
            if n:
                trace.append("%d vector load%s" % (n, "" if n == 1 else "s"))
                n = 0
            if e[0] == "wait":
                trace.append("WAIT " + e[1])
            elif e[0] == "fma":
                trace.append("first multiply-add")
    if not ends:
        return None
    return (min(e[0] for e in ends), max(e[1] for e in ends)), late, trace


def block_events(instrs, karg, kernarg_base, stop_at_fma):
    """Events of one block; karg (the scalar pairs holding the kernel-argument pointer) is updated in place."""
    ev = []
    for s in instrs:
        m = FMA.match(s)
        if m and stop_at_fma:
            ev.append(("fma", m.group(1)))
            break
        m = SLOAD.match(s)
        if m:
            dwords = int(m.group(2) or m.group(3) or 1)
            dest, base, off = m.group(4).rstrip(","), m.group(5), m.group(6).rstrip(",")
            ev.append(("sload", dwords, dest, base, off, _regs(base) in karg))
            d = _regs(dest)
            if d:
                karg -= {p for p in karg if not (p[1] < d[0] or p[0] > d[1])}
            continue
        m = VLOAD.match(s)
        if m:
            ev.append(("vload", m.group(1), m.group(2)))
            continue
        m = LDSLOAD.match(s)
        if m:
            ev.append(("ldsload", m.group(1)))
            continue
        m = WAIT.match(s)
        if m:
            ev.append(("wait", m.group(1).strip()))
            continue
        parts = s.split(None, 1)   # register bookkeeping: copies of the kernel-argument pointer, and writes that end one
        if len(parts) == 2 and parts[0].startswith(("s_", "v_readfirstlane", "v_readlane")) and \
                not parts[0].startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop")):
            ops = [o.strip() for o in parts[1].split(",")]
            d = _regs(ops[0])
            if d:
                src = _regs(ops[1]) if len(ops) > 1 else None
                copy = parts[0] == "s_mov_b64" and src in karg
                karg -= {p for p in karg if not (p[1] < d[0] or p[0] > d[1])}
                if copy:
                    karg.add(d)
    return ev


def prologue_events(body, kernarg_base=0):
    """Events of the prologue in execution order: ("label", name) | ("sload", dwords, dest, base, offset, from_kernarg)
       | ("vload", mnemonic, dest) | ("ldsload", mnemonic) | ("wait", text) | ("fma", mnemonic); and the per-way wait counts
       {"scalar": (min, max), "vector": (min, max)}."""
    blocks = basic_blocks(body)
    if not blocks:
        return [], {"scalar": (0, 0), "vector": (0, 0)}
    order, target, fwd = prologue_blocks(blocks)
    karg = {(kernarg_base, kernarg_base + 1)}
    ev, per_block = [], {}
    for i in order:
        e = block_events(blocks[i][1], karg, kernarg_base, i == target)
        per_block[i] = e
        ev.append(("label", blocks[i][0] or ("entry" if i == 0 else "(fallthrough)")))
        ev += e
    # dependent waits per way: state = (scalar load pending, vector load pending) -> (fewest, most) waits so far
    counts = {}
    for kind, loads, counter in (("scalar", ("sload",), "lgkmcnt"), ("vector", ("vload",), "vmcnt")):
        best = {0: {False: (0, 0)}}
        inset = set(order)
        for i in order:
            states = best.get(i)
            if not states:
                continue
            out = {}
            for pending, (lo, hi) in states.items():
                for e in per_block[i]:
                    if e[0] in loads:
                        pending = True
                    elif e[0] == "wait" and counter in e[1] and pending:
                        lo, hi, pending = lo + 1, hi + 1, False
                o = out.get(pending)
                out[pending] = (min(lo, o[0]), max(hi, o[1])) if o else (lo, hi)
            if i == target:
                los = [v[0] for v in out.values()]
                his = [v[1] for v in out.values()]
                counts[kind] = (min(los), max(his))
                break
            for v in fwd[i]:
                if v not in inset:
                    continue
                dst = best.setdefault(v, {})
                for pending, (lo, hi) in out.items():
                    o = dst.get(pending)
                    dst[pending] = (min(lo, o[0]), max(hi, o[1])) if o else (lo, hi)
        counts.setdefault(kind, (0, 0))
    return ev, counts


def kernarg_loads_after_first_lgkm_wait(ev):
    """Scalar loads from the kernel-argument pointer that come after the first wait on lgkmcnt."""
    late, waited = [], False
    for e in ev:
        if e[0] == "wait" and "lgkmcnt" in e[1]:
            waited = True
        elif e[0] == "sload" and e[5] and waited:
            late.append(e)
    return late


def wide_scalar_loads(ev, dwords=8):
    return [e for e in ev if e[0] == "sload" and e[1] >= dwords]


def format_events(ev):
    out, group, kind = [], [], None

    def flush():
        nonlocal group, kind
        if not group:
            return
        if kind == "sload":
            out.append("  scalar loads (%d):" % len(group))
            for e in group:
                out.append("    %-12s <- %s + %s  (%d dword%s)" % (e[2], "kernarg" if e[5] else e[3], e[4], e[1], "" if e[1] == 1 else "s"))
        elif kind == "vload":
            out.append("  vector loads (%d): %s" % (len(group), ", ".join(sorted({e[1] for e in group}))))
        else:
            out.append("  LDS loads (%d)" % len(group))
        group, kind = [], None

    label = None   # printed only in front of a block that has something to show
    for e in ev:
        if e[0] == "label":
            flush()
            label = e[1]
            continue
        if label is not None:
            out.append(" %s:" % label)
            label = None
        if e[0] in ("sload", "vload", "ldsload"):
            if kind != e[0]:
                flush()
                kind = e[0]
            group.append(e)
            continue
        flush()
        if e[0] == "wait":
            out.append("  WAIT  s_waitcnt " + e[1])
        elif e[0] == "fma":
            out.append("  first multiply-add: " + e[1])
    flush()
    return out


def report_whole(text, wanted):
    kernels = split_kernels(text)
    lines = []
    for sym in sorted(kernels):
        if wanted and not any(w in sym for w in wanted):
            continue
        lines.append("== " + sym)
        w = whole_counts(kernels[sym][0])
        if w is None:
            lines += ["  no multiply-add on a way to s_endpgm", ""]
            continue
        (lo, hi), late, trace = w
        lines.append("  vector loads and vmcnt waits to s_endpgm, blocks in execution order: " + "; ".join(trace))
        lines.append("  dependent vector waits over the ways through the first multiply-add to s_endpgm, fewest .. most: %d .. %d" % (lo, hi))
        lines.append("  vector loads behind the first multiply-add: %d" % late)
        lines.append("")
    return lines


def report(text, wanted):
    kernels = split_kernels(text)
    lines = []
    for sym in sorted(kernels):
        if wanted and not any(w in sym for w in wanted):
            continue
        body, base = kernels[sym]
        ev, counts = prologue_events(body, base)
        lines.append("== " + sym)
        lines += format_events(ev)
        lines.append("  kernel-argument loads behind the first lgkmcnt wait: %d" % len(kernarg_loads_after_first_lgkm_wait(ev)))
        lines.append("  scalar loads of 8 or more dwords: %d" % len(wide_scalar_loads(ev)))
        lines.append("  dependent waits before the first multiply-add, fewest .. most over the ways there: scalar %d .. %d, vector %d .. %d"
                     % (counts["scalar"] + counts["vector"]))
        lines.append("")
    return lines


# the B = 64 f32 decode step of bench.py: attention, QKV / out-proj / FC1 / FC2, head, greedy tail
BENCH = (
    ("attn_paged.hip", ("attn_paged_kernelILi64ELb0ELb0E",)),
    ("gemm_skinny.hip", ("gemm_skinny_kernelILi0ELb1ELi2ELi1ELb0ELi2E", "gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi2E",
                         "gemm_skinny_kernelILi2ELb1ELi2ELi1ELb0ELi2E", "gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi8E")),
    ("head_gemm.hip", ("head_balanced_kernelILi2ELi2ELb0ELb0E",)),
    ("step_tail.hip", ("argmax_advance_embed_kernel",)),
)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", nargs="?")
    ap.add_argument("kernels", nargs="*")
    ap.add_argument("--asm", action="store_true", help="FILE is an assembly listing")
    ap.add_argument("--bench", action="store_true", help="the seven kernels of the benchmark step")
    ap.add_argument("--csrc", default=CSRC, help="source directory for --bench")
    ap.add_argument("--whole", action="store_true", help="walk to s_endpgm: dependent vector waits and vector loads behind the first multiply-add")
    a = ap.parse_args()
    rep = report_whole if a.whole else report
    if a.bench:
        for f, syms in BENCH:
            print("# " + f)
            print("\n".join(rep(compile_to_asm(os.path.join(a.csrc, f)), syms)))
        return 0
    if not a.file:
        ap.error("FILE or --bench")
    if a.asm:
        with open(a.file) as f:
            text = f.read()
    else:
        text = compile_to_asm(a.file)
    print("\n".join(rep(text, a.kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
