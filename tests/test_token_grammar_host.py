"""Token grammars on the host: TokenGrammar's checks and walks against a brute-force automaton, the track grammar of
generate_music.grammar against the detokeniser, and RowSampling's new trailing argument.  No GPU."""
import numpy as np
import pytest

from mgea import synth
from mgea.decoder import RowSampling, TokenGrammar

ENDPOINT_PROMPT = ["[START_SEQUENCE]", "[BPM] 120", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]


def random_grammar(rng, vocab, n_state, n_class, p_ban=0.5):
    """random class_of, random next with every entry banned with probability p_ban, repaired so that every state admits a class
    that has an id"""
    class_of = rng.integers(0, n_class, vocab).astype(np.int32)
    nxt = rng.integers(0, n_state, (n_state, n_class)).astype(np.int32)
    nxt[rng.random((n_state, n_class)) < p_ban] = -1
    populated = np.unique(class_of)
    for s in range(n_state):
        if not (nxt[s, populated] >= 0).any():
            nxt[s, rng.choice(populated)] = rng.integers(0, n_state)
    return TokenGrammar(class_of, nxt)


def test_check_refuses_each_cap_and_bad_entries():
    ok = TokenGrammar(np.zeros(10, np.int32), np.zeros((1, 1), np.int32))
    ok.check(10)
    with pytest.raises(ValueError, match="n_class 4097"):
        TokenGrammar(np.zeros(10, np.int32), np.zeros((1, 4097), np.int32)).check(10)
    with pytest.raises(ValueError, match="n_state 4097"):
        TokenGrammar(np.zeros(10, np.int32), np.zeros((4097, 1), np.int32)).check(10)
    with pytest.raises(ValueError, match="cells"):
        TokenGrammar(np.zeros(10, np.int32), np.zeros((2048, 513), np.int32)).check(10)
    TokenGrammar(np.zeros(10, np.int32), np.zeros((2048, 512), np.int32)).check(10)   # exactly 1 << 20 cells
    with pytest.raises(ValueError, match=r"class_of must be \[11\]"):
        ok.check(11)
    with pytest.raises(ValueError, match=r"class_of\[3\] = 2"):
        TokenGrammar(np.array([0, 1, 1, 2], np.int32), np.zeros((1, 2), np.int32)).check(4)
    with pytest.raises(ValueError, match=r"class_of\[0\] = -1"):
        TokenGrammar(np.array([-1, 1], np.int32), np.zeros((1, 2), np.int32)).check(2)
    with pytest.raises(ValueError, match=r"next\[1\]\[0\] = 2"):
        TokenGrammar(np.array([0, 1], np.int32), np.array([[0, 1], [2, 0]], np.int32)).check(2)
    with pytest.raises(ValueError, match=r"next\[0\]\[1\] = -2"):
        TokenGrammar(np.array([0, 1], np.int32), np.array([[0, -2], [1, 0]], np.int32)).check(2)
    with pytest.raises(ValueError, match=r"\[n_state, n_class\]"):
        TokenGrammar(np.zeros(4, np.int32), np.zeros(4, np.int32))


def test_check_refuses_a_state_whose_admitted_classes_are_all_empty():
    # class 2 has no id: state 1 admits only it
    class_of = np.array([0, 1, 1, 0], np.int32)
    nxt = np.array([[0, 1, -1], [-1, -1, 0]], np.int32)
    with pytest.raises(ValueError, match="state 1 admits no class that has an id"):
        TokenGrammar(class_of, nxt).check(4)
    nxt[1, 0] = 1
    TokenGrammar(class_of, nxt).check(4)
    with pytest.raises(ValueError, match="state 0 admits"):
        TokenGrammar(class_of, np.full((1, 3), -1, np.int32)).check(4)


def test_walks_agree_with_brute_force():
    rng = np.random.default_rng(5)
    for vocab, n_state, n_class in ((40, 3, 1), (300, 4, 7), (500, 8, 33)):
        g = random_grammar(rng, vocab, n_state, n_class)
        g.check(vocab)
        table = {(s, i): int(g.next[s][int(g.class_of[i])]) for s in range(n_state) for i in range(vocab)}
        for s in range(n_state):
            allowed = g.allowed(s)
            assert allowed.dtype == bool and allowed.shape == (vocab,) and allowed.any()
            for i in range(vocab):
                assert g.step(s, i) == table[(s, i)]
                assert bool(allowed[i]) == (table[(s, i)] >= 0)
        for _ in range(50):
            ids = rng.integers(0, vocab, 12).tolist()
            s0 = int(rng.integers(0, n_state))
            s, lax, legal = s0, s0, True
            for i in ids:
                n = table[(lax, i)]
                lax = n if n >= 0 else lax
                if legal:
                    n = table[(s, i)]
                    legal, s = n >= 0, n if n >= 0 else s
            assert g.accepts(ids, s0) == legal
            assert g.run(ids, s0, strict=False) == lax
            if legal:
                assert g.run(ids, s0) == s == lax
            else:
                with pytest.raises(ValueError, match="banned in state"):
                    g.run(ids, s0)
        assert g.run([], 2 % n_state) == 2 % n_state and g.accepts([], 0)


@pytest.mark.parametrize("vocab", [300, 8324])
def test_track_grammar_tables(vocab):
    from generate_music.grammar import HEAD, OPEN, start_state, track_grammar
    from generate_music.midi import note_re
    tok2id = synth.decoder_vocab(vocab, with_eos=True)
    names = list(tok2id)
    g = track_grammar(tok2id)
    g.check(vocab)
    starts = sorted({float(note_re.match(t).group(2)) for t in names if note_re.match(t)})
    K = len(starts)
    assert (g.n_state, g.n_class) == (K + 2, K + 3) and (HEAD, OPEN) == (0, 1)
    for t, i in tok2id.items():
        m = note_re.match(t)
        want = starts.index(float(m.group(2))) if m else K if t.startswith("[INSTRUMENT]") else K + 1 if t == "[END_SEQUENCE]" else K + 2
        assert g.class_of[i] == want, t
    inst, eos, other = tok2id["[INSTRUMENT] Flute"], tok2id["[END_SEQUENCE]"], tok2id["[BPM] 120"]
    note = {k: next(i for t, i in tok2id.items() if note_re.match(t) and float(note_re.match(t).group(2)) == starts[k]) for k in range(K)}
    assert g.step(HEAD, inst) == OPEN and g.step(HEAD, other) == HEAD and g.step(HEAD, eos) == -1 and g.step(HEAD, note[0]) == -1
    assert g.step(OPEN, inst) == -1 and g.step(OPEN, eos) == -1 and g.step(OPEN, other) == -1
    for k in range(K):
        assert g.step(OPEN, note[k]) == 2 + k
        assert g.step(2 + k, inst) == OPEN and g.step(2 + k, eos) == 2 + k and g.step(2 + k, other) == -1
        for k2 in range(K):
            assert g.step(2 + k, note[k2]) == (2 + k2 if k2 >= k else -1)
    free = track_grammar(tok2id, monotone_starts=False)
    assert all(free.step(2 + K - 1, note[k]) == 2 + k for k in range(K))
    assert start_state(g, [tok2id[t] for t in ENDPOINT_PROMPT]) == OPEN
    assert start_state(g, [tok2id[t] for t in ENDPOINT_PROMPT[:3]]) == HEAD
    # a vocabulary without [END_SEQUENCE]: the EOS class is empty, and nothing else changes
    no_eos = track_grammar(synth.decoder_vocab(vocab))
    assert no_eos.n_class == g.n_class and not (no_eos.class_of == K + 1).any()
    with pytest.raises(ValueError, match="state 1 admits no class"):   # no notes at all: OPEN admits nothing
        track_grammar({t: i for i, t in enumerate(n for n in names if not note_re.match(n))})


@pytest.mark.parametrize("vocab", [300, 8324])
def test_sequences_drawn_from_allowed_survive_the_detokeniser(vocab):
    """200 sequences of 40 ids drawn uniformly from allowed(), from OPEN (the prompt named the instrument): the detokeniser keeps
    every token that is not [END_SEQUENCE], no track's START goes back, and every instrument has a note.  The 40-id cut is the
    test's, not the grammar's: an instrument that is the very last id of a sequence is followed by nothing, so the last property is
    checked on the sequence without that id."""
    from generate_music.grammar import OPEN, track_grammar
    from generate_music.midi import tokens_to_instruments
    tok2id = synth.decoder_vocab(vocab, with_eos=True)
    names = list(tok2id)
    g = track_grammar(tok2id)
    rng = np.random.default_rng(7)
    n_inst = n_eos = 0
    for _ in range(200):
        s, ids = OPEN, []
        for _ in range(40):
            i = int(rng.choice(np.flatnonzero(g.allowed(s))))
            ids.append(i)
            s = g.step(s, i)
            assert s >= 0
        assert g.accepts(ids, OPEN) and g.run(ids, OPEN) == s
        toks = [names[i] for i in ids]
        if toks[-1].startswith("[INSTRUMENT]"):
            toks = toks[:-1]
        tracks = tokens_to_instruments(["[INSTRUMENT] Violin"] + toks)
        kept = len(tracks) - 1 + sum(len(t.notes) for t in tracks)
        assert kept == sum(t != "[END_SEQUENCE]" for t in toks)
        for t in tracks:
            assert len(t.notes) >= 1
            st = [n.start for n in t.notes]
            assert st == sorted(st)
        n_inst += len(tracks) - 1
        n_eos += toks.count("[END_SEQUENCE]")
    assert n_inst > 0 and (vocab > 300 or n_eos > 0)   # the draws reach the instrument branch (and, in the small vocabulary, the EOS)


def test_broken_sequences_are_rejected():
    from generate_music.grammar import HEAD, OPEN, track_grammar
    tok2id = synth.decoder_vocab(300, with_eos=True)
    g = track_grammar(tok2id)
    note = lambda p, s, d: tok2id[f"[NOTE] [PITCH:{p}] [START:{s}] [END:{round(s + d, 2)}] [DURATION:{d}]"]
    early, late = note("C2", 0.0, 0.25), note("C2", 0.25, 0.25)
    violin, flute, eos = tok2id["[INSTRUMENT] Violin"], tok2id["[INSTRUMENT] Flute"], tok2id["[END_SEQUENCE]"]
    assert g.accepts([early, late, late, flute, early, eos], OPEN)
    assert not g.accepts([late, early], OPEN)                 # a START that goes back
    assert not g.accepts([early], HEAD)                       # a note before any instrument
    assert not g.accepts([violin, flute], HEAD)               # instrument - instrument
    assert not g.accepts([flute], OPEN)
    assert not g.accepts([early, tok2id["[BPM] 120"]], OPEN)  # a control token inside a track
    assert not g.accepts([eos], OPEN)                         # an empty track cannot end the piece
    assert g.accepts([late, flute, early], OPEN)              # a new track starts over
    assert g.accepts([late, early], OPEN) is False and track_grammar(tok2id, monotone_starts=False).accepts([late, early], OPEN)


def test_row_sampling_takes_the_state_as_its_eleventh_argument():
    import dataclasses
    old = RowSampling(0.9, 20, 0.92, 1.1, 2, 0, 7, None, None, 3)
    assert old.grammar_state is None and old.min_new_tokens == 3
    assert RowSampling().grammar_state is None
    assert RowSampling(0.9, 20, 0.92, 1.1, 2, 0, 7, None, None, 3, 5).grammar_state == 5
    r = RowSampling(grammar_state=4)
    assert r.grammar_state == 4 and dataclasses.replace(r, max_new_tokens=9).grammar_state == 4
    assert dataclasses.replace(r, grammar_state=None).grammar_state is None
    r.check(0, 100, 10)


# ---------------------------------------------------------------------------------------------------------- drop-in and serving
class GrammarStubEngine:
    """What generate_requests needs of a DecoderEngine, plus the engine's grammar slot."""

    def __init__(self, vocab=64, max_batch=8, max_ctx=128):
        self.vocab, self.max_batch, self.max_ctx = vocab, max_batch, max_ctx
        self.grammar, self.uploads, self.calls = None, 0, []

    def set_grammar(self, g):
        self.grammar, self.uploads = g, self.uploads + 1

    def generate_rows(self, prompts, rows, n_steps=None):
        import torch
        self.calls.append(dict(prompts=[list(p) for p in prompts], rows=list(rows), grammar=self.grammar))
        return torch.zeros(len(prompts), n_steps, dtype=torch.int32)


def grammar_stub_model():
    import generate_music.generate as gen
    gen.set_vocab(synth.decoder_vocab(64, with_eos=True))
    m = gen.GPTWithKV(64, 128, 64, 2, 1)
    m.engine = GrammarStubEngine()
    return m, gen


def test_entry_points_start_every_row_in_the_state_of_its_prompt():
    from generate_music.grammar import HEAD, OPEN, track_grammar
    m, gen = grammar_stub_model()
    g = track_grammar(gen.tok2id)
    prompts = [ENDPOINT_PROMPT, ENDPOINT_PROMPT[:3]]
    gen.generate_requests(m, prompts, max_len=12, top_k=1, seed=0, grammar=g)
    gen.generate_requests(m, prompts[:1], max_len=12, top_k=1, seed=0, grammar=g)
    assert m.engine.uploads == 1 and m.engine.grammar is g          # the object set there is not uploaded again
    assert [r.grammar_state for r in m.engine.calls[0]["rows"]] == [OPEN, HEAD]
    gen.generate_requests(m, prompts, max_len=12, top_k=1, seed=0)
    assert [r.grammar_state for r in m.engine.calls[2]["rows"]] == [None, None]
    gen.generate_batch_grammar(m, prompts, max_len=12, top_k=1, seed=0, grammar=g)
    rows = m.engine.calls[3]["rows"]
    assert [r.grammar_state for r in rows] == [OPEN, HEAD] and [r.stream for r in rows] == [None, None]
    out = gen.sample_kvcache_grammar(m, ENDPOINT_PROMPT, max_len=9, top_k=1, seed=0, grammar=g)
    assert m.engine.calls[4]["rows"][0].grammar_state == OPEN and len(out) == 9


def test_batcher_serves_one_grammar_object_per_batch():
    from generate_music.grammar import track_grammar
    from mgea.decoder import TokenGrammar
    from mgea.serve import RequestBatcher
    m, gen = grammar_stub_model()
    g1, g2 = track_grammar(gen.tok2id), track_grammar(gen.tok2id, monotone_starts=False)
    b = RequestBatcher(m, autostart=False)
    with pytest.raises(ValueError, match="class_of must be"):
        b.submit(ENDPOINT_PROMPT, 12, grammar=TokenGrammar(np.zeros(3, np.int32), np.zeros((1, 1), np.int32)))
    futs = [b.submit(ENDPOINT_PROMPT, 12, grammar=g) for g in (g1, g1, g2, None, None)]
    b.start()
    for f in futs:
        assert len(f.result(timeout=30)) == 12
    b.close()
    assert [f.batch_rows for f in futs] == [2, 2, 1, 2, 2] and b.stats()["rows_per_generation"] == [2, 1, 2]
    assert [c["grammar"] for c in m.engine.calls[:2]] == [g1, g2]
    assert [r.grammar_state for r in m.engine.calls[2]["rows"]] == [None, None]
