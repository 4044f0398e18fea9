"""Classifier-free guidance, host side (no device): the unconditional prompt, the pair rules of mgea_decoder_generate_rows_guided as
ValueErrors naming the row, and the shadow-row packing of DecoderEngine.generate_guided (mgea.decoder.pack_guided)."""
import math

import numpy as np
import pytest
import torch

from generate_music.guidance import unconditional_prompt
from mgea.decoder import RowSampling, check_guidance, pack_guided


def test_unconditional_prompt_drops_the_emotion_tokens():
    prompt = ["[START_SEQUENCE]", "[BPM] 120.0", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]
    assert unconditional_prompt(prompt) == ["[START_SEQUENCE]", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]
    assert unconditional_prompt(["[START_SEQUENCE]", "[INSTRUMENT] Violin"]) == ["[START_SEQUENCE]", "[INSTRUMENT] Violin"]
    # wherever they stand, however many there are; a note token that merely mentions a key is not one
    assert unconditional_prompt(["[BPM] 90.0", "a", "[KEY_SIGNATURE] F# minor", "[BPM] 60.0", "x [BPM] 1"]) == ["a", "x [BPM] 1"]
    assert unconditional_prompt(tuple(prompt)) == unconditional_prompt(prompt)
    with pytest.raises(ValueError, match="nothing but"):
        unconditional_prompt(["[BPM] 120.0", "[KEY_SIGNATURE] C major"])
    with pytest.raises(ValueError):
        unconditional_prompt([])


def test_pair_rules_name_the_row():
    check_guidance([3, -1, -1, -1, 2], [1.5, 0, 0, 0, 0.0], 5)
    check_guidance([-1, -1], [math.nan, -3.0], 2)          # the scale of a row that is not conditional is not read
    check_guidance([1, -1], [1.0, 0.0], 2)                 # scale 1 is legal
    with pytest.raises(ValueError, match=r"row 1: shadow_row 3 outside \[-1, 3\)"):
        check_guidance([-1, 3, -1], [0, 1, 0], 3)
    with pytest.raises(ValueError, match=r"row 0: shadow_row -2 outside"):
        check_guidance([-2, -1], [1, 1], 2)
    with pytest.raises(ValueError, match="row 1: a row cannot be its own shadow"):
        check_guidance([-1, 1], [1, 1], 2)
    with pytest.raises(ValueError, match="row 0: its shadow row 1 is conditional itself"):
        check_guidance([1, 2, -1], [1, 1, 1], 3)
    with pytest.raises(ValueError, match="row 1: row 2 is already the shadow of row 0"):
        check_guidance([2, 2, -1], [1, 1, 1], 3)
    for bad in (math.nan, math.inf, -0.5, 1e39):           # 1e39 is inf as a float32
        with pytest.raises(ValueError, match="row 0: guidance scale .* finite and >= 0"):
            check_guidance([1, -1], [bad, 0], 2)
    with pytest.raises(ValueError, match="3 rows"):
        check_guidance([1, -1], [1, 0], 3)


def test_shadow_rows_are_packed_behind_the_callers_rows():
    rows = [RowSampling(1.0, 20, seed=b) for b in range(4)]
    prompts = [[1, 2, 3], [4, 5], [6], [7, 8, 9, 10]]
    negs = [[1], None, [6, 6], None]
    p, r, shadow, scales, forced = pack_guided(prompts, negs, rows, [1.5, 9.0, 0.0, math.nan], 8, [[5], [], None, [1, 2]])
    assert p == prompts + [[1], [6, 6]]
    assert r[:4] == rows and r[4] is rows[0] and r[5] is rows[2], "a shadow row carries its conditional row's settings"
    assert shadow == [4, -1, 5, -1, -1, -1] and scales == [1.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert forced == [[5], [], None, [1, 2], None, None]
    # one scale for all, tensors for prompts and forced ids, no pair at all
    p, r, shadow, scales, forced = pack_guided(torch.tensor([[1, 2], [3, 4]]), [torch.tensor([2]), [4]], rows[:2], 3, 4,
                                               torch.tensor([[7, -1, 7], [-1, -1, 9]]))
    assert p == [[1, 2], [3, 4], [2], [4]] and shadow == [2, 3, -1, -1] and scales == [3.0, 3.0, 0.0, 0.0]
    assert forced.tolist() == [[7, -1, 7], [-1, -1, 9], [-1, -1, -1], [-1, -1, -1]]
    p, r, shadow, scales, forced = pack_guided(prompts, None, rows, 2.0, 4)
    assert p == prompts and r == rows and shadow == [-1] * 4 and forced is None
    scale_arr = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    assert pack_guided(prompts, negs, rows, scale_arr, 6)[3] == [1.0, 0.0, 3.0, 0.0, 0.0, 0.0]


def test_packing_refusals_name_the_row():
    rows = [RowSampling() for _ in range(3)]
    prompts = [[1], [2], [3]]
    with pytest.raises(ValueError, match=r"row 2: its shadow row 4 does not fit: 3 prompts \+ 2 negative prompts exceed max_batch 4"):
        pack_guided(prompts, [[1], None, [3]], rows, 1.5, 4)
    pack_guided(prompts, [[1], None, [3]], rows, 1.5, 5)
    with pytest.raises(ValueError, match="row 1: guidance scale -1.0 must be finite and >= 0"):
        pack_guided(prompts, [None, [2], None], rows, [math.nan, -1.0, 0.0], 8)
    with pytest.raises(ValueError, match="row 0: empty negative prompt"):
        pack_guided(prompts, [[], None, None], rows, 1.5, 8)
    with pytest.raises(ValueError, match="3 prompts but 2 negative prompts"):
        pack_guided(prompts, [None, None], rows, 1.5, 8)
    with pytest.raises(ValueError, match="3 prompts but 2 sampler rows"):
        pack_guided(prompts, None, rows[:2], 1.5, 8)
    with pytest.raises(ValueError, match="guidance_scale: 2 values for 3 prompts"):
        pack_guided(prompts, None, rows, [1.0, 2.0], 8)
    with pytest.raises(ValueError, match="3 prompts but 1 force_ids rows"):
        pack_guided(prompts, [[1], None, None], rows, 1.5, 8, [[1]])


def test_the_c_abi_declares_the_guided_entry_points():
    from mgea import _lib
    for name in ("mgea_decoder_generate_rows_guided", "mgea_decoder_guidance_info", "mgea_op_guidance_mix"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name)
    assert _lib.RowGuidance(shadow_row=3, scale=1.5).shadow_row == 3 and [f[0] for f in _lib.RowGuidance._fields_] == ["shadow_row", "scale"]
    import ctypes
    assert ctypes.sizeof(_lib.RowGuidance) == 8
