"""tools/prologue_chain.py --whole: the walk to s_endpgm on a listing written here, and -- where hipcc exists -- the decode GEMMs as
compiled.  What the kernels are held to: every operand chunk of the wave (8, 32, 12 loads) is requested before the first MFMA, no
load is issued inside the K chain and its vmcnt waits only count down; behind the last MFMA stands the epilogue's own round trip
(bias, c1, the residual float4; QKV's page-table look-up where the pool has no allocation rule), kept there on purpose: requested
with the operands it measured slower (profiles/epilogue_inputs_ab.txt).  So a wave waits for vector memory
once or twice (the threads without a first-pass epilogue item: once), QKV at most three times (the table way).
Only load, wait and MFMA mnemonics are looked at."""
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music-generation-emotion-adaptive_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("prologue_chain", os.path.join(ROOT, "tools", "prologue_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# `drip`: a workgroup outside the grid leaves at once (no wait: that way does not count).  The others request two operands, wait for
# the first, multiply, request the third BEHIND the multiply-add and wait twice more (the second of these waits has nothing new to
# wait for).  One way then looks a table entry up and waits for it; the other does not.  Stores never count.
# `front`: every load in front of the multiply-add, waits that only count down.
# `plain`: no multiply-add at all.
LISTING = """
	.text
	.globl	drip
drip:                                   ; @drip
; %bb.0:
	s_load_dwordx4 s[4:7], s[0:1], 0x0
	s_waitcnt lgkmcnt(0)
	s_cmp_gt_u32 s4, 7
	s_cbranch_scc1 .LBB0_4
; %bb.1:
	global_load_dwordx4 v[4:7], v0, s[6:7]
	global_load_dwordx4 v[8:11], v0, s[6:7] offset:1024
	s_waitcnt vmcnt(1)
	v_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
	global_load_dwordx4 v[12:15], v0, s[6:7] offset:2048
	s_waitcnt vmcnt(1)
	v_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]
	s_waitcnt vmcnt(0)
	v_mfma_f32_16x16x4_f32 v[0:3], v12, v13, v[0:3]
	s_cmp_eq_u32 s5, 0
	s_cbranch_scc1 .LBB0_3
; %bb.2:
	global_load_dword v16, v0, s[6:7] offset:4096
	s_waitcnt vmcnt(0)
	v_add_u32_e32 v0, v0, v16
.LBB0_3:
	global_store_dwordx4 v0, v[0:3], s[6:7]
	s_waitcnt vmcnt(0)
.LBB0_4:
	s_endpgm
.Lfunc_end0:
	.globl	front
front:                                  ; @front
; %bb.0:
	global_load_dwordx4 v[4:7], v0, s[6:7]
	global_load_dwordx4 v[8:11], v0, s[6:7] offset:1024
	global_load_dwordx4 v[12:15], v0, s[6:7] offset:2048
	s_waitcnt vmcnt(2)
	v_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
	s_waitcnt vmcnt(1)
	v_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]
	s_waitcnt vmcnt(0)
	ds_read_b128 v[4:7], v20
	s_waitcnt lgkmcnt(0)
	global_store_dwordx4 v0, v[0:3], s[6:7]
	s_endpgm
.Lfunc_end1:
	.globl	plain
plain:                                  ; @plain
; %bb.0:
	global_load_dword v1, v0, s[6:7]
	s_waitcnt vmcnt(0)
	global_store_dword v0, v1, s[6:7]
	s_endpgm
.Lfunc_end2:
"""


def test_whole_walk_on_a_written_listing():
    pc = _tool()
    kernels = pc.split_kernels(LISTING)
    assert sorted(kernels) == ["drip", "front", "plain"]
    (lo, hi), late, trace = pc.whole_counts(kernels["drip"][0])
    assert (lo, hi) == (2, 3), (lo, hi)          # operands, the third operand; the table entry on one way only
    assert late == 2                             # the third operand and the table entry
    assert trace[:3] == ["2 vector loads", "WAIT vmcnt(1)", "first multiply-add"], trace
    (lo, hi), late, trace = pc.whole_counts(kernels["front"][0])
    assert (lo, hi) == (1, 1) and late == 0
    assert trace == ["3 vector loads", "WAIT vmcnt(2)", "first multiply-add", "WAIT vmcnt(1)", "WAIT vmcnt(0)"], trace
    assert pc.whole_counts(kernels["plain"][0]) is None
    text = "\n".join(pc.report_whole(LISTING, []))
    assert "fewest .. most: 2 .. 3" in text and "vector loads behind the first multiply-add: 2" in text
    assert "fewest .. most: 1 .. 1" in text and "no multiply-add" in text
    # the prologue report of the same listing is what it was: up to the first multiply-add only
    _, counts = pc.prologue_events(*kernels["drip"])
    assert counts["vector"] == (1, 1)


@functools.lru_cache(maxsize=None)
def _skinny():
    pc = _tool()
    if pc.find_hipcc() is None:
        pytest.skip("no hipcc")
    return pc.split_kernels(pc.compile_to_asm(os.path.join(CSRC, "gemm_skinny.hip")))


def _whole(sym):
    kernels = _skinny()
    match = [k for k in kernels if sym in k]
    assert len(match) == 1, f"{sym}: {match}"
    w = _tool().whole_counts(kernels[match[0]][0])
    assert w is not None, sym
    return w


@pytest.mark.parametrize("sym,late,waits", [("gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi2E", 2, (1, 2)),     # out-projection: bias, residual
                                            ("gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi8E", 2, (1, 2)),     # FC2: bias, residual
                                            ("gemm_skinny_kernelILi2ELb1ELi2ELi1ELb0ELi2E", 2, (1, 2)),     # FC1: c2, c1
                                            ("gemm_skinny_kernelILi0ELb1ELi2ELi1ELb0ELi2E", 3, (1, 3))])    # QKV: c2, c1, page table
def test_only_the_epilogue_round_trip_stands_behind_the_first_mfma(sym, late, waits):
    """behind the first MFMA: the epilogue's two inputs (QKV: and the page table's look-up on the way without the allocation rule),
    nothing else; the waves without a first-pass item wait once, the others once more (QKV's table way: a third time)"""
    (lo, hi), n_late, trace = _whole(sym)
    assert n_late == late, f"{sym}: {n_late} vector loads behind the first MFMA: {trace}"
    assert (lo, hi) == waits, f"{sym}: {lo} .. {hi} dependent vector waits: {trace}"


@pytest.mark.parametrize("sym,loads", [("gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi2E", 8),      # out-projection: 2 chunks x (2 W + 2 A)
                                       ("gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi8E", 32),     # FC2: 8 chunks
                                       ("gemm_skinny_kernelILi2ELb1ELi2ELi1ELb0ELi2E", 12),     # FC1: 2 chunks x (2 W + 4 A)
                                       ("gemm_skinny_kernelILi0ELb1ELi2ELi1ELb0ELi2E", 12)])    # QKV
def test_operand_chunks_are_all_requested_before_the_first_mfma(sym, loads):
    """every operand load of the wave stands in front of the first MFMA (with the statistics and, for QKV, the two lengths), and from
    there to the last MFMA no load is issued and the vmcnt waits only count down: the K chain is one round trip"""
    _, _, trace = _whole(sym)
    at = trace.index("first multiply-add")
    before = sum(int(t.split()[0]) for t in trace[:at] if t.endswith(("vector load", "vector loads")))
    assert before >= loads, f"{sym}: {before} vector loads in front of the first MFMA, {loads} operand loads expected: {trace}"
    chain = []
    for t in trace[at + 1:]:
        if not t.startswith("WAIT"):
            break
        chain.append(int(t.split("vmcnt(")[1].split(")")[0]))
    assert len(chain) >= 2 and chain == sorted(chain, reverse=True), f"{sym}: waits behind the first MFMA {chain}: {trace}"
