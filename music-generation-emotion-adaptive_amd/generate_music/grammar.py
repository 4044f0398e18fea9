"""Token grammars for the decoder's sampler: which whole-line token may FOLLOW which.

Host-side string work only.  The result is a mgea.decoder.TokenGrammar -- a finite automaton over token classes -- for
DecoderEngine.set_grammar / RowSampling.grammar_state; the sampler masks every step's logits with the row's current state and the
step's tail moves the state on the device (include/mgea.h, mgea_decoder_set_grammar).  Build-defined: the reference samples the raw
vocabulary.

Why: the detokeniser (generate_music/midi.py, api_cache.py:208-221) keeps an `[INSTRUMENT] X` token (it opens a track) and a
`[NOTE] ...` token (it adds a note to the open track) and drops everything else -- a note drawn before any instrument included; an
instrument followed directly by another one leaves an empty track, and the START times inside a track can jump backwards.  The
training data (midi_test/midi_tokenization.py) never looks like that: one `[INSTRUMENT]` line, then that instrument's notes, per
track, then `[END_SEQUENCE]`.  A static logit bias (generate_music.constraints) can ban ids; it cannot say what may follow what.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from mgea.decoder import TokenGrammar

from .constraints import EOS_TOKEN
from .midi import note_re

HEAD, OPEN = 0, 1   # states: no instrument yet; an instrument was just named; 2 + k: the track's last note started at value k


def track_grammar(tok2id: Dict[str, int], monotone_starts: bool = True) -> TokenGrammar:
    """The grammar of the training data's tracks.
    Classes: one per distinct note START value, ascending, 0 .. K - 1; INSTRUMENT = K; EOS = K + 1 (empty if the vocabulary has no
    [END_SEQUENCE]); OTHER = K + 2 (every control token).
    States: HEAD = 0 (no instrument yet) admits INSTRUMENT (-> OPEN) and OTHER (stays); OPEN = 1 (an instrument was just named)
    admits notes only, any START (-> 2 + k); 2 + k (the track's last note started at value k) admits the notes of class >= k when
    monotone_starts, else every note (-> 2 + k'), INSTRUMENT (-> OPEN) and EOS (stays).  OTHER is banned outside HEAD.
    ValueError (TokenGrammar.check) if the vocabulary has no instrument or no note, or more START values than the caps allow."""
    vocab = max(tok2id.values()) + 1 if tok2id else 0
    starts: Dict[int, float] = {}
    for tok, i in tok2id.items():
        m = note_re.match(tok)
        if m:
            starts[i] = float(m.group(2))
    values = sorted(set(starts.values()))
    K = len(values)
    rank = {v: k for k, v in enumerate(values)}
    INSTRUMENT, EOS, OTHER = K, K + 1, K + 2
    class_of = np.full(vocab, OTHER, np.int32)
    for tok, i in tok2id.items():
        if i in starts:
            class_of[i] = rank[starts[i]]
        elif tok.startswith("[INSTRUMENT]"):
            class_of[i] = INSTRUMENT
        elif tok == EOS_TOKEN:
            class_of[i] = EOS
    nxt = np.full((K + 2, K + 3), -1, np.int32)
    nxt[HEAD, INSTRUMENT] = OPEN
    nxt[HEAD, OTHER] = HEAD
    nxt[OPEN, :K] = 2 + np.arange(K)
    for k in range(K):
        lo = k if monotone_starts else 0
        nxt[2 + k, lo:K] = 2 + np.arange(lo, K)
        nxt[2 + k, INSTRUMENT] = OPEN
        nxt[2 + k, EOS] = 2 + k
    g = TokenGrammar(class_of, nxt)
    g.check(vocab)
    return g


def start_state(grammar: TokenGrammar, prompt_ids: Sequence[int]) -> int:
    """The state a generation starts in after its prompt: the walk from HEAD in which a token the grammar bans leaves the state
    alone (the prompt is given, not drawn).  The endpoint's prompt -- [START_SEQUENCE], bpm, key, instruments -- ends in OPEN."""
    return grammar.run(prompt_ids, HEAD, strict=False)
