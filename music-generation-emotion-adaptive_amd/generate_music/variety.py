"""Penalty classes for the decoder: which ATTRIBUTE of a note a windowed penalty counts.

Host-side string work only.  An id of this vocabulary is a whole line `[NOTE] [PITCH:p] [START:s] [END:e] [DURATION:d]` with the
note's absolute START, so an id recurs only as a literal duplicate and the id-level repetition_penalty is nearly inert for what a
listener calls repetition: the same pitches, the same rhythm.  token_classes maps every id to the class of one attribute; the engine
counts the classes of a row's last `window` generated ids and lowers (or, with negative values, raises) every id of a counted class
(mgea.decoder.ClassPenalty, DecoderEngine.set_penalty_classes; the rule: include/mgea.h, mgea_row_class_penalty).  Build-defined: the
reference has no such control.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from .midi import note_name_to_number, note_re

KINDS = ("pitch", "pitch_class", "duration", "pitch_duration", "id")


def token_classes(tok2id: Dict[str, int], by: str = "pitch") -> np.ndarray:
    """int32 [vocab], vocab = the largest id + 1: the class of every note token, classes numbered densely from 0 in ascending order of
    their key, and -1 for every other id (instruments, [END_SEQUENCE], control tokens, ids no token names): never counted, never
    penalised.  by:
      "pitch"           the MIDI number of the note's pitch name (midi.note_name_to_number: C#4 and D-4 are one class)
      "pitch_class"     that number mod 12
      "duration"        the DURATION value
      "pitch_duration"  the pair (MIDI number, DURATION)
      "id"              the id itself: the frequency / presence penalty over ids of other engines
    ValueError for another `by` and for a vocabulary without a note."""
    if by not in KINDS:
        raise ValueError(f"token_classes: by = {by!r}, expected one of {KINDS}")
    vocab = max(tok2id.values()) + 1 if tok2id else 0
    keys = {}
    for tok, i in tok2id.items():
        m = note_re.match(tok)
        if not m:
            continue
        pitch = note_name_to_number(m.group(1))
        dur = float(m.group(4))
        keys[i] = {"pitch": pitch, "pitch_class": pitch % 12, "duration": dur, "pitch_duration": (pitch, dur), "id": i}[by]
    if not keys:
        raise ValueError("token_classes: the vocabulary has no note token")
    rank = {k: c for c, k in enumerate(sorted(set(keys.values())))}
    class_of = np.full(vocab, -1, np.int32)
    for i, k in keys.items():
        class_of[i] = rank[k]
    return class_of
