"""Classifier-free guidance for the music decoder: what the unconditional side of a pair is.

The emotion of a request reaches the decoder only through the control tokens of its prompt -- `[START_SEQUENCE]`, the `[BPM] ...`
token, the `[KEY_SIGNATURE] ...` token, then the instruments (api_cache.py:203).  The negative prompt of a guided generation is that
prompt without the two emotion tokens: the same piece for the same instruments, with nothing said about tempo and key.  The engine runs
it as a shadow row and draws every id from scale * logp(prompt) + (1 - scale) * logp(negative prompt)
(mgea.decoder.DecoderEngine.generate_guided).  Pure host code.
"""
from __future__ import annotations

from typing import List, Sequence

EMOTION_PREFIXES = ("[BPM]", "[KEY_SIGNATURE]")


def unconditional_prompt(tokens: Sequence[str]) -> List[str]:
    """The prompt without its `[BPM]` and `[KEY_SIGNATURE]` tokens, everything else in order.  ValueError if nothing is left (a
    generation needs a token to start from)."""
    out = [t for t in tokens if not str(t).startswith(EMOTION_PREFIXES)]
    if not out:
        raise ValueError("unconditional_prompt: the prompt holds nothing but [BPM] / [KEY_SIGNATURE] tokens")
    return out
