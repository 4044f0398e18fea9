"""Emotion transitions for the music decoder: a piece whose conditioning follows the emotions of a text.

The reference splits a text into sentences and labels each one (emotion_analysis.inference.analyze_emotion_transitions, "not done
yet" upstream) and has nothing downstream that uses the result: a generation has one emotion for its whole length, carried by the
`[BPM] ...` and `[KEY_SIGNATURE] ...` tokens of its prompt (api_cache.py:203).  Here every sentence's emotion gives one VARIANT of the
prompt -- the same instruments, another tempo and key -- and the engine swaps the prompt's cached K | V for the next variant's when
the generation reaches the next segment (mgea.decoder.DecoderEngine.generate_scheduled; the rule: include/mgea.h, mgea_row_schedule).
Under the track grammar a segment is a range of note START classes, so the switch follows musical time inside every track.  Pure
host code.
"""
from __future__ import annotations

from typing import List, Sequence

from .guidance import EMOTION_PREFIXES

MAX_SEGMENTS = 8   # mgea.decoder.SCHEDULE_MAX_SEGMENTS


def _emotion_tokens(params) -> List[str]:
    """[bpm token, key token] of one parameter set: an EATS mapping (its "bpm" and "key" go through closest_bpm_token /
    normalize_key_signature, as the endpoint's do) or a ready (bpm token, key token) pair"""
    if isinstance(params, dict):
        from . import generate as gen
        pair = [gen.closest_bpm_token(params["bpm"]), gen.normalize_key_signature(params["key"])]
    else:
        pair = [str(t) for t in params]
    if len(pair) != 2 or not pair[0].startswith(EMOTION_PREFIXES[0]) or not pair[1].startswith(EMOTION_PREFIXES[1]):
        raise ValueError(f"transition_prompts: {params!r} is not a ([BPM] token, [KEY_SIGNATURE] token) pair")
    return pair


def transition_prompts(prompt_tokens: Sequence[str], params_list) -> List[List[str]]:
    """One prompt variant per parameter set: prompt_tokens with its `[BPM]` token and its `[KEY_SIGNATURE]` token replaced by the
    set's.  Everything else -- the instruments above all -- stays, so the variants have one length by construction.  ValueError for
    no set or more than 8, and for a prompt that does not hold exactly one token of each kind."""
    prompt_tokens = [str(t) for t in prompt_tokens]
    params_list = list(params_list)
    if not 1 <= len(params_list) <= MAX_SEGMENTS:
        raise ValueError(f"transition_prompts: {len(params_list)} segments outside [1, {MAX_SEGMENTS}]")
    where = [[i for i, t in enumerate(prompt_tokens) if t.startswith(p)] for p in EMOTION_PREFIXES]
    if any(len(w) != 1 for w in where):
        raise ValueError("transition_prompts: the prompt must hold exactly one [BPM] and one [KEY_SIGNATURE] token")
    out = []
    for params in params_list:
        v = list(prompt_tokens)
        for (i,), tok in zip(where, _emotion_tokens(params)):
            v[i] = tok
        out.append(v)
    return out


def _shares(shares, n: int) -> List[float]:
    shares = [1.0] * n if shares is None else [float(s) for s in shares]
    if len(shares) != n or n < 1 or any(not (s > 0 and s < float("inf")) for s in shares):
        raise ValueError(f"shares {shares} must be {n} positive finite numbers")
    return shares


def start_thresholds(grammar, shares) -> List[int]:
    """The thresholds (grammar STATES, for RowSchedule(key=1)) of len(shares) segments under generate_music.grammar.track_grammar:
    its K START classes, ascending in time, are cut in proportion to shares, and segment s begins at state 2 + k_s, k_s = the first
    class of the segment (at least s: no segment is empty while K allows it).  HEAD and OPEN lie below every threshold: a track
    that opens is in segment 0 until its first note.  ValueError if the grammar has no START class."""
    K = int(grammar.n_state) - 2
    shares = _shares(shares, len(shares))
    if K < 1:
        raise ValueError("start_thresholds: the grammar has no note START classes")
    total, acc, out, n = sum(shares), 0.0, [], len(shares)
    for s, share in enumerate(shares[:-1]):
        acc += share
        lo, hi = s + 1, K - 1 - (n - 2 - s)   # one class at least for every segment before and behind the boundary
        k = min(max(int(round(K * acc / total)), lo), max(hi, 1)) if lo <= hi else min(lo, K - 1)
        out.append(2 + max(k, out[-1] - 2 if out else 0))
    return out


def step_thresholds(n_steps: int, shares) -> List[int]:
    """The thresholds (step indices, for RowSchedule(key=0)) of len(shares) segments over n_steps decode steps, cut in proportion to
    shares."""
    shares = _shares(shares, len(shares))
    total, acc, out = sum(shares), 0.0, []
    for share in shares[:-1]:
        acc += share
        out.append(max(int(round(int(n_steps) * acc / total)), out[-1] if out else 0))
    return out
