"""Emotion blends for the music decoder: one piece conditioned on several emotions at once.

The classifier returns a distribution over its labels (emotion_analysis.inference.predict_top_k_labels), and a generation used to be
conditioned on the arg-max alone: a text that is 55 % joy and 30 % nostalgia got the music of a text that is 99 % joy.  Here every
kept emotion gives one variant of the prompt -- the same instruments, that emotion's `[BPM]` and `[KEY_SIGNATURE]` tokens -- and the
engine runs the variants as one group of rows that draws every id from sum_k w_k * logp(variant k)
(mgea.decoder.DecoderEngine.generate_blended; the rule: include/mgea.h, mgea_row_blend).  Classifier-free guidance on top of a blend
is one more member, the prompt without its emotion tokens, with weight 1 - scale.  Pure host code.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

from .guidance import unconditional_prompt
from .transitions import transition_prompts

MAX_ROWS = 8   # mgea.decoder.BLEND_MAX_ROWS


def blend_prompts(prompt_tokens: Sequence[str], params_list, unconditional: bool = False) -> List[List[str]]:
    """One prompt per EATS parameter set (transitions.transition_prompts: the same instruments, the set's `[BPM]` and
    `[KEY_SIGNATURE]` tokens), the first the group's leader; unconditional=True appends the prompt without its emotion tokens
    (guidance.unconditional_prompt) as the last member.  ValueError for no set and for more than 8 members in all."""
    params_list = list(params_list)
    if not 1 <= len(params_list) + int(bool(unconditional)) <= MAX_ROWS:
        raise ValueError(f"blend_prompts: {len(params_list)} emotions{' + the unconditional prompt' if unconditional else ''} outside "
                         f"[1, {MAX_ROWS}] rows")
    out = transition_prompts(prompt_tokens, params_list)
    if unconditional:
        out.append(unconditional_prompt([str(t) for t in prompt_tokens]))
    return out


def blend_weights(probs, guidance_scale: Optional[float] = None) -> List[float]:
    """The weights of a group from the emotions' probabilities: normalised to sum 1; with a guidance scale s they are multiplied by s
    and one more weight, 1 - s, is appended for the unconditional member (blend_prompts(..., unconditional=True)) -- the sum stays 1.
    ValueError for no probability, more than 8 members in all, a negative or non-finite probability, a zero sum and a scale that is
    not finite and >= 0."""
    probs = [float(p) for p in probs]
    if not 1 <= len(probs) + int(guidance_scale is not None) <= MAX_ROWS:
        raise ValueError(f"blend_weights: {len(probs)} probabilities{'' if guidance_scale is None else ' + the unconditional member'} outside "
                         f"[1, {MAX_ROWS}] rows")
    if any(not (math.isfinite(p) and p >= 0) for p in probs) or not sum(probs) > 0:
        raise ValueError(f"blend_weights: probabilities {probs} must be finite, >= 0 and not all 0")
    total = sum(probs)
    w = [p / total for p in probs]
    if guidance_scale is None:
        return w
    s = float(guidance_scale)
    if not (math.isfinite(s) and s >= 0):
        raise ValueError(f"blend_weights: guidance scale {guidance_scale} must be finite and >= 0")
    return [s * v for v in w] + [1.0 - s]
