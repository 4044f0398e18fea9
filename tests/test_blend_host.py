"""Emotion blends, host side (no device): the group rules of mgea_decoder_generate_rows_blended as ValueErrors naming the row
(mgea.decoder.check_blend), the member packing of DecoderEngine.generate_blended (pack_blended), the prompts and weights of a
blended request (generate_music.blend), the C ABI's declarations, and the plan of a blended generation
(tests/native/blend_plan_test.cpp, a stand-alone host program over csrc/gen_plan.h)."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from generate_music.blend import blend_prompts, blend_weights
from mgea.decoder import BLEND_MAX_ROWS, RowSampling, check_blend, pack_blended

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


# ---------------------------------------------------------------------------------------------------------- the group rules
def test_group_rules_name_the_row():
    assert BLEND_MAX_ROWS == 8
    check_blend([0, -1, 3, 3, -1, 0], [0.5, math.nan, 1.25, -0.25, 9.0, 0.5], 6)   # the weight of an ungrouped row is not read
    check_blend([3, 3, 3, 3], [0.0, 0.0, 2.0, -1.0], 4)                          # zeros and negative weights; a leader that is the last row
    check_blend([-1, -1], [1, 1], 2)
    check_blend([0] * 8 + [-1], [0.125] * 8 + [0], 9)                            # eight rows
    check_blend([0, 0], [0.5, 0.5009], 2)                                        # within 1e-3 of 1
    with pytest.raises(ValueError, match=r"row 1: leader 3 outside \[-1, 3\)"):
        check_blend([0, 3, 0], [0.5, 1, 0.5], 3)
    with pytest.raises(ValueError, match=r"row 0: leader -2 outside"):
        check_blend([-2, -1], [1, 1], 2)
    with pytest.raises(ValueError, match=r"row 0: its leader row 1 does not name itself \(leader -1\)"):
        check_blend([1, -1, 1], [0.5, 0, 0.5], 3)
    with pytest.raises(ValueError, match=r"row 0: its leader row 1 does not name itself \(leader 2\)"):
        check_blend([1, 2, 2], [0.5, 0.5, 0.5], 3)
    with pytest.raises(ValueError, match=r"row 2: a group of 1 row"):
        check_blend([-1, -1, 2], [0, 0, 1.0], 3)
    with pytest.raises(ValueError, match=r"row 8: the group of leader row 0 has more than 8 rows"):
        check_blend([0] * 9, [1.0] + [0.0] * 8, 9)
    for bad in (math.nan, math.inf, -math.inf, 1e39):          # 1e39 is inf as a float32
        with pytest.raises(ValueError, match="row 1: weight .* must be finite"):
            check_blend([0, 0], [0.5, bad], 2)
    for w, total in ((0.4, "0.9"), (0.6, "1.1")):
        with pytest.raises(ValueError, match=f"row 1: the weights of its group sum to {total}"):
            check_blend([-1, 1, 1], [0, 0.5, w], 3)
    # a row both grouped and paired: the conditional side and the shadow side
    check_blend([0, 0, -1, -1], [0.5, 0.5, 0, 0], 4, shadow_rows=[-1, -1, 3, -1])
    with pytest.raises(ValueError, match="row 0 is in a blend group and in a guidance pair"):
        check_blend([0, 0, -1, -1], [0.5, 0.5, 0, 0], 4, shadow_rows=[3, -1, -1, -1])
    with pytest.raises(ValueError, match="row 1 is in a blend group and in a guidance pair"):
        check_blend([0, 0, -1, -1], [0.5, 0.5, 0, 0], 4, shadow_rows=[-1, -1, 1, -1])
    with pytest.raises(ValueError, match="3 rows"):
        check_blend([0, 0], [0.5, 0.5], 3)


# ---------------------------------------------------------------------------------------------------------- the packing
def test_members_are_packed_behind_the_callers_rows():
    rows = [RowSampling(1.0, 20, seed=b) for b in range(3)]
    groups = [[[1, 2, 3], [1, 9, 3], [1, 8, 3]], [[4, 5]], [[6], [7]]]
    weights = [[0.6, 0.3, 0.1], [123.0], [1.5, -0.5]]
    p, r, leader, weight, forced = pack_blended(groups, weights, rows, 8, [[5, 5], [], [1]])
    assert p == [[1, 2, 3], [4, 5], [6], [1, 9, 3], [1, 8, 3], [7]]
    assert leader == [0, -1, 2, 0, 0, 2] and weight == [0.6, 0.0, 1.5, 0.3, 0.1, -0.5]
    assert r[:3] == rows
    for b, l in enumerate(leader):
        assert l < 0 or r[b] is r[l], "a member carries its leader's settings"
    assert forced == [[5, 5], [], [1], [5, 5], [5, 5], [1]], "a member is told its leader's ids"
    # tensors for prompts and forced ids; a bare id list is a group of one; no group at all
    p, r, leader, weight, forced = pack_blended([torch.tensor([[1, 2], [3, 4]]), [5, 6]], [[0.5, 0.5], [1.0]], rows[:2], 4,
                                                torch.tensor([[7, -1, 7], [-1, -1, 9]]))
    assert p == [[1, 2], [5, 6], [3, 4]] and leader == [0, -1, 0] and weight == [0.5, 0.0, 0.5]
    assert forced.tolist() == [[7, -1, 7], [-1, -1, 9], [7, -1, 7]]
    p, r, leader, weight, forced = pack_blended([[[1]], [[2]]], [[1.0], [1.0]], rows[:2], 2)
    assert p == [[1], [2]] and r == rows[:2] and leader == [-1, -1] and forced is None
    # eight prompts fill a group
    p, r, leader, weight, _ = pack_blended([[[i] for i in range(8)]], [[0.125] * 8], rows[:1], 8)
    assert leader == [0] * 8 and len(p) == 8


def test_packing_refusals_name_the_group():
    rows = [RowSampling() for _ in range(2)]
    groups = [[[1], [2], [3]], [[4], [5]]]
    weights = [[0.5, 0.25, 0.25], [0.5, 0.5]]
    with pytest.raises(ValueError, match=r"group 1: its member row 4 does not fit: 5 prompts in 2 groups exceed max_batch 4"):
        pack_blended(groups, weights, rows, 4)
    pack_blended(groups, weights, rows, 5)
    with pytest.raises(ValueError, match=r"group 0: 9 prompts outside \[1, 8\]"):
        pack_blended([[[i] for i in range(9)]], [[1.0] + [0.0] * 8], rows[:1], 16)
    with pytest.raises(ValueError, match="group 1: 3 weights for 2 prompts"):
        pack_blended(groups, [weights[0], [0.5, 0.25, 0.25]], rows, 8)
    with pytest.raises(ValueError, match="group 0: empty prompt"):
        pack_blended([[[1], []], [[4]]], [[0.5, 0.5], [1.0]], rows, 8)
    with pytest.raises(ValueError, match="row 0: the weights of its group sum to 0.9"):
        pack_blended(groups, [[0.5, 0.25, 0.15], [0.5, 0.5]], rows, 8)
    with pytest.raises(ValueError, match="row 2: weight nan must be finite"):   # group 0's second prompt is row 2 of the batch
        pack_blended(groups, [[0.5, math.nan, 0.25], [0.5, 0.5]], rows, 8)
    with pytest.raises(ValueError, match="2 prompt groups but 1 sampler rows"):
        pack_blended(groups, weights, rows[:1], 8)
    with pytest.raises(ValueError, match="2 prompt groups but 1 force_ids rows"):
        pack_blended(groups, weights, rows, 8, [[1]])


# ---------------------------------------------------------------------------------------------------------- prompts and weights
PROMPT = ["[START_SEQUENCE]", "[BPM] 120.0", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]


def test_blend_prompts_and_weights_have_one_length_by_construction():
    params = [("[BPM] 120.0", "[KEY_SIGNATURE] C major"), ("[BPM] 60.0", "[KEY_SIGNATURE] A minor"), ("[BPM] 90.0", "[KEY_SIGNATURE] G major")]
    got = blend_prompts(PROMPT, params)
    assert got[0] == PROMPT and len(got) == 3 and all(len(g) == len(PROMPT) for g in got)
    assert got[1] == ["[START_SEQUENCE]", "[BPM] 60.0", "[KEY_SIGNATURE] A minor", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]
    w = blend_weights([0.55, 0.30, 0.05])
    assert len(w) == len(got) and abs(sum(w) - 1) < 1e-12 and w == pytest.approx([0.55 / 0.9, 0.30 / 0.9, 0.05 / 0.9])
    assert blend_weights([3]) == [1.0]
    # with guidance: one more member, the prompt without its emotion tokens, with weight 1 - s
    got_u = blend_prompts(PROMPT, params, unconditional=True)
    assert got_u[:3] == got and got_u[3] == ["[START_SEQUENCE]", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]
    for s in (0.0, 1.0, 1.5, 3.0):
        ws = blend_weights([0.55, 0.30, 0.05], s)
        assert len(ws) == len(got_u) and ws[-1] == 1.0 - s and ws[:3] == pytest.approx([s * v for v in w])
        assert abs(sum(ws) - 1) < 1e-12
        leader = [0] * 4
        check_blend(leader, ws, 4)
    assert blend_weights([1.0], 1.5) == [1.5, -0.5]   # classifier-free guidance is the group (s, 1 - s)


def test_blend_prompts_and_weights_refuse_more_than_eight_rows():
    pair = ("[BPM] 60.0", "[KEY_SIGNATURE] A minor")
    assert len(blend_prompts(PROMPT, [pair] * 8)) == 8 and len(blend_prompts(PROMPT, [pair] * 7, unconditional=True)) == 8
    with pytest.raises(ValueError, match="9 emotions"):
        blend_prompts(PROMPT, [pair] * 9)
    with pytest.raises(ValueError, match="8 emotions \\+ the unconditional prompt"):
        blend_prompts(PROMPT, [pair] * 8, unconditional=True)
    with pytest.raises(ValueError):
        blend_prompts(PROMPT, [])
    assert len(blend_weights([1] * 8)) == 8 and len(blend_weights([1] * 7, 2.0)) == 8
    with pytest.raises(ValueError, match="9 probabilities"):
        blend_weights([0.1] * 9)
    with pytest.raises(ValueError, match="8 probabilities \\+ the unconditional member"):
        blend_weights([0.1] * 8, 1.5)
    for bad in ([], [0.0, 0.0], [0.5, -0.1], [math.nan], [math.inf]):
        with pytest.raises(ValueError):
            blend_weights(bad)
    for s in (math.nan, math.inf, -0.5):
        with pytest.raises(ValueError, match="guidance scale"):
            blend_weights([0.5, 0.5], s)


# ---------------------------------------------------------------------------------------------------------- the C ABI and the surface
def test_the_c_abi_declares_the_blended_entry_points():
    from mgea import _lib
    hdr = open(os.path.join(ROOT, "include", "mgea.h")).read()
    lib = _lib.load()
    for name in ("mgea_decoder_generate_rows_blended", "mgea_decoder_blend_info", "mgea_op_blend_mix"):
        assert name + "(" in hdr and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "#define MGEA_BLEND_MAX_ROWS 8" in hdr and _lib.BLEND_MAX_ROWS == 8
    assert C.sizeof(_lib.RowBlend) == 8 and [f[0] for f in _lib.RowBlend._fields_] == ["leader", "weight"]
    assert _lib.RowBlend(leader=3, weight=0.25).leader == 3
    trunc, blend = (_lib.PROTOTYPES[f"mgea_decoder_generate_rows_{n}"][1] for n in ("truncated", "blended"))
    assert blend[:len(trunc) - 1] == trunc[:-1] and blend[-2:] == [C.POINTER(_lib.RowBlend), C.c_void_p]


def test_surface():
    import api_shim
    import generate_music.generate as gen
    from mgea import ops
    from mgea.decoder import DecoderEngine
    four = ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"]
    for f in (gen.sample_kvcache_blended, gen.generate_requests_blended, api_shim.create_blended_app):
        sig = inspect.signature(f).parameters
        assert all(n in sig and sig[n].default is None for n in four), f.__name__
    assert list(inspect.signature(gen.sample_kvcache_blended).parameters)[:8] == ["model", "prompts", "weights", "max_len", "temperature",
                                                                                 "top_k", "top_p", "repetition_penalty"]
    sig = inspect.signature(api_shim.create_blended_app).parameters
    assert (sig["top_emotions"].default, sig["min_prob"].default, sig["guidance_scale"].default) == (3, 0.05, None)
    assert list(inspect.signature(DecoderEngine.generate_blended).parameters)[:7] == ["self", "prompt_groups", "weights", "rows", "n_steps",
                                                                                     "force_ids", "scored"]
    assert callable(ops.blend_mix) and callable(DecoderEngine.blend_info)

    class Small:
        max_batch = 2
    with pytest.raises(ValueError, match="max_batch=2 is too small"):
        api_shim.create_blended_app(Small(), 64)
    with pytest.raises(ValueError, match="max_batch=2 is too small"):
        api_shim.create_blended_app(Small(), 64, top_emotions=2, guidance_scale=1.5)
    with pytest.raises(ValueError, match="top_emotions 9"):
        api_shim.create_blended_app(Small(), 64, top_emotions=9)
    with pytest.raises(ValueError, match="guidance_scale"):
        api_shim.create_blended_app(Small(), 64, guidance_scale=-1.0)
    with pytest.raises(ValueError, match="min_prob"):
        api_shim.create_blended_app(Small(), 64, top_emotions=2, min_prob=1.5)


# ---------------------------------------------------------------------------------------------------------- the plan
def test_blend_plan_native(tmp_path):
    """tests/native/blend_plan_test.cpp: kind.blended, never GREEDY, both flags for a pair and a group, every refusal, the capped
    call, NULL / all -1 records => the truncated plan.  A stand-alone host program; with AddressSanitizer and UBSan where there is
    no GPU."""
    exe = str(tmp_path / "blend_plan_test")
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *san,
                           os.path.join(ROOT, "tests", "native", "blend_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "blend_plan ok" and r.stderr == "", r.stdout + r.stderr
