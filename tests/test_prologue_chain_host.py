"""tools/prologue_chain.py: its parser on a listing written here, and -- where hipcc exists -- the prologues of the decode step's
kernels as compiled: q no longer comes through the scalar path, the lengths are one wait, and every kernel-argument load stands in
front of the first wait.  Only load, wait and branch mnemonics are looked at."""
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


# Two kernels.  `late`: the second argument load stands behind the first wait, and a 16-dword scalar load feeds the FMA.  `loop`: the
# compiler's block order -- the block that ends the kernel (with an FMA of its own) stands in front of the loop; one table look-up is
# on one way to the loop only.
LISTING = """
	.text
	.globl	late
late:                                   ; @late
; %bb.0:
	s_load_dwordx2 s[4:5], s[0:1], 0x0
	s_waitcnt lgkmcnt(0)
	s_load_dword s6, s[0:1], 0x10
	s_load_dwordx16 s[8:23], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	v_mov_b32_e32 v1, s8
	v_fma_f32 v0, v1, v1, v0
	s_endpgm
.Lfunc_end0:
	.globl	loop
loop:                                   ; @loop
; %bb.0:
	s_mov_b64 s[2:3], s[0:1]
	s_load_dwordx4 s[4:7], s[2:3], 0x0
	s_load_dword s8, s[0:1], 0x10
	s_waitcnt lgkmcnt(0)
	s_load_dword s9, s[4:5], 0x0
	global_load_dword v1, v0, s[6:7]
	s_waitcnt lgkmcnt(0)
	s_cmp_eq_u32 s8, 0
	s_cbranch_scc1 .LBB1_3
; %bb.1:
	s_cmp_gt_i32 s9, 0
	s_cbranch_scc1 .LBB1_4
.LBB1_2:
	v_fma_f32 v3, v3, v3, v3
	global_store_dword v0, v3, s[6:7]
	s_endpgm
.LBB1_3:
	s_load_dword s10, s[6:7], 0x4
	s_waitcnt lgkmcnt(0)
.LBB1_4:
	global_load_dwordx4 v[4:7], v0, s[6:7] offset:16
	s_waitcnt vmcnt(1)
	v_fma_f32 v3, v1, v2, v3
	s_add_i32 s9, s9, -1
	s_cmp_lg_u32 s9, 0
	s_cbranch_scc1 .LBB1_4
	s_branch .LBB1_2
.Lfunc_end1:
"""


def test_parser_on_a_written_listing():
    pc = _tool()
    kernels = pc.split_kernels(LISTING)
    assert sorted(kernels) == ["late", "loop"]

    ev, counts = pc.prologue_events(*kernels["late"])
    assert [e[0] for e in ev if e[0] != "label"] == ["sload", "wait", "sload", "sload", "wait", "fma"]
    late = pc.kernarg_loads_after_first_lgkm_wait(ev)
    assert [(e[2], e[4]) for e in late] == [("s6", "0x10")]              # the one from s[0:1]; the x16 load has another base
    assert [e[1] for e in pc.wide_scalar_loads(ev)] == [16]
    assert counts["scalar"] == (2, 2) and counts["vector"] == (0, 0)

    ev, counts = pc.prologue_events(*kernels["loop"])
    kinds = [e[0] for e in ev if e[0] != "label"]
    assert kinds[-1] == "fma" and kinds.count("fma") == 1
    # the end block's FMA (in front of the loop in the listing) is not the prologue's end, and its store block is not on the way
    assert [e[1] for e in ev if e[0] == "label"][-1] == ".LBB1_4"
    sl = [e for e in ev if e[0] == "sload"]
    assert [e[5] for e in sl] == [True, True, False, False]              # s[2:3] is a copy of the kernel-argument pointer
    assert pc.kernarg_loads_after_first_lgkm_wait(ev) == [] and pc.wide_scalar_loads(ev) == []
    assert counts["scalar"] == (2, 3)                                    # arguments, length; the table look-up on one way only
    assert counts["vector"] == (1, 1)
    text = "\n".join(pc.report(LISTING, ["loop"]))
    assert "scalar 2 .. 3, vector 1 .. 1" in text and "kernarg + 0x10" in text


@functools.lru_cache(maxsize=None)
def _compiled(name):
    pc = _tool()
    if pc.find_hipcc() is None:
        pytest.skip("no hipcc")
    return pc.split_kernels(pc.compile_to_asm(os.path.join(CSRC, name)))


def _events(fname, sym):
    pc = _tool()
    kernels = _compiled(fname)
    match = [k for k in kernels if sym in k]
    assert len(match) == 1, f"{sym}: {match}"
    return pc.prologue_events(*kernels[match[0]])


def test_attention_q_leaves_the_scalar_path():
    """attn_paged_kernel<64, false, false>, both page-id paths (they are two ways through the same code): no scalar load of 8 or more
    dwords; in front of the first FMA a wave waits for scalar data at most for the arguments, for the lengths (ctx_len and lens
    together) and, with page ids from the table, for one look-up.  Fewest = computed page ids: 2.  The walk cannot know that the
    table look-up of wave 0's early K page and the one of the other waves' first page exclude each other (`wave == 0 && zsplit == 0`
    and its negation), so the most it finds on one way is 4 where a wave meets 3."""
    pc = _tool()
    ev, counts = _events("attn_paged.hip", "attn_paged_kernelILi64ELb0ELb0E")
    assert pc.wide_scalar_loads(ev) == []
    assert pc.kernarg_loads_after_first_lgkm_wait(ev) == []
    assert counts["scalar"][0] <= 2, counts
    assert counts["scalar"][1] <= 4, counts
    # the look-ups themselves: two sites, each one dword from a base that is not the argument pointer, besides the two lengths
    other = [e for e in ev if e[0] == "sload" and not e[5]]
    assert len(other) <= 4 and all(e[1] == 1 for e in other), other


@pytest.mark.parametrize("fname,sym", [
    ("step_tail.hip", "argmax_advance_embed_kernel"),
    ("head_gemm.hip", "head_balanced_kernelILi2ELi2ELb0ELb0E"),
    ("gemm_skinny.hip", "gemm_skinny_kernelILi0ELb1ELi2ELi1ELb0ELi2E"),
    ("gemm_skinny.hip", "gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi2E"),
    ("gemm_skinny.hip", "gemm_skinny_kernelILi2ELb1ELi2ELi1ELb0ELi2E"),
    ("gemm_skinny.hip", "gemm_skinny_kernelILi1ELb0ELi1ELi1ELb0ELi8E"),
])
def test_argument_block_is_one_batch(fname, sym):
    """every scalar load from the kernel-argument pointer precedes the first lgkmcnt wait"""
    pc = _tool()
    ev, _ = _events(fname, sym)
    assert any(e[0] == "sload" and e[5] for e in ev), "no kernel-argument load found: the walk lost the pointer"
    late = pc.kernarg_loads_after_first_lgkm_wait(ev)
    assert late == [], f"{sym}: argument loads behind the first wait: {[(e[2], e[4]) for e in late]}"
