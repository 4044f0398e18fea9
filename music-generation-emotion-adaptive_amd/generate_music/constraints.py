"""Vocabulary constraints for the decoder's sampler: which of the whole-line tokens a generation may draw.

Host-side string work only.  The result is a float32 [vocab] logit bias (0 = untouched, -inf = banned, a finite value = a soft
penalty) for DecoderEngine.generate_biased(..., logit_bias=) / RowSampling.logit_bias; the sampler adds it to the logits after the
repetition penalty (include/mgea.h, mgea_row_logits).  Build-defined: the reference samples the raw vocabulary.

Why: the detokeniser (generate_music/midi.py, api_cache.py:208-221) keeps `[INSTRUMENT] X` and `[NOTE] ...` tokens and drops
everything else, so every control token drawn after the prompt is a wasted step; and the emotion's key (EATS.get_music_params)
otherwise reaches the model as one prompt token only.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Set

import numpy as np

from .midi import note_name_to_number, note_re

MAJOR = (0, 2, 4, 5, 7, 9, 11)
MINOR = (0, 2, 3, 5, 7, 8, 10)   # natural minor
EOS_TOKEN = "[END_SEQUENCE]"

_key_re = re.compile(r"^([A-Ga-g])([#\-b]*)$")


def pitch_class(name: str) -> int:
    """Pitch class 0..11 of a pitch name without octave ("F#", "B-", "Eb"), spelled as in midi.note_name_to_number."""
    if not _key_re.match(name):
        raise ValueError(f"Improper pitch name: {name}")
    return note_name_to_number(name + "4") % 12


def scale_pitch_classes(key: str) -> Set[int]:
    """The seven pitch classes of a key: "D Major", "B♭ Major", "C# Minor" (EATS strings) or "[KEY_SIGNATURE] B- major" (the
    normalised token).  Major = tonic + {0,2,4,5,7,9,11}; minor = the natural minor, tonic + {0,2,3,5,7,8,10}."""
    s = key.replace("[KEY_SIGNATURE]", "").replace("♭", "-").replace("♯", "#").strip()
    parts = s.split()
    if len(parts) != 2 or parts[1].lower() not in ("major", "minor"):
        raise ValueError(f"not a key: {key!r} (want '<tonic> major|minor')")
    tonic = pitch_class(parts[0])
    steps = MAJOR if parts[1].lower() == "major" else MINOR
    return {(tonic + d) % 12 for d in steps}


def classify_vocab(tok2id: Dict[str, int]) -> Dict[str, object]:
    """The vocabulary by what the detokeniser does with a token: {"notes": {id: pitch class}, "instruments": [ids], "eos": id or -1,
    "control": [ids of everything else]}."""
    notes: Dict[int, int] = {}
    instruments: List[int] = []
    control: List[int] = []
    eos = -1
    for tok, i in tok2id.items():
        m = note_re.match(tok)
        if m:
            notes[i] = note_name_to_number(m.group(1)) % 12
        elif tok.startswith("[INSTRUMENT]"):
            instruments.append(i)
        elif tok == EOS_TOKEN:
            eos = i
        else:
            control.append(i)
    return dict(notes=notes, instruments=sorted(instruments), eos=eos, control=sorted(control))


def logit_bias(tok2id: Dict[str, int], key: Optional[str] = None, notes_only: bool = True,
               out_of_scale: float = -np.inf) -> np.ndarray:
    """float32 [vocab]: -inf on the control ids when notes_only (notes, instruments and [END_SEQUENCE] stay), and `out_of_scale`
    (-inf, or a finite penalty <= 0 typically) ADDED on the notes whose pitch class is outside `key`'s scale (key None: no scale
    constraint).  ValueError if no note, instrument or control token stays admissible."""
    out_of_scale = float(out_of_scale)
    if np.isnan(out_of_scale) or out_of_scale == np.inf:
        raise ValueError("out_of_scale must be finite or -inf")
    cls = classify_vocab(tok2id)
    vocab = max(tok2id.values()) + 1 if tok2id else 0
    bias = np.zeros(vocab, np.float32)
    if notes_only:
        bias[cls["control"]] = -np.inf
    if key is not None:
        scale = scale_pitch_classes(key)
        out = [i for i, pc in cls["notes"].items() if pc not in scale]
        bias[out] += np.float32(out_of_scale)
    admissible = np.isfinite(bias)
    if cls["eos"] >= 0:
        admissible[cls["eos"]] = False   # a generation that can only end is not one
    if not admissible.any():
        raise ValueError("the constraint leaves no admissible token besides [END_SEQUENCE]")
    return bias
