"""Per-row token grammars on the MI355X: the GRAMMAR sampler against the fp32 restatement of the host-masked row, a one-state
grammar against the static bias it equals, stateful greedy generations against the oracle, sampled generations that hold the track
grammar, the grammar form's graphs, forced ids, the fp16 engine, the errors and the endpoints.

Tolerances are those of tests/test_gpu_logit_bias.py: probabilities atol 2e-6 / rtol 1e-4; a greedy generation may leave the oracle's
only where the oracle's own processed top-2 gap is below NEAR_TIE, and at most one row of a test may use that.  The seeds of the
oracle tests were chosen on the CPU, by running the oracle loop alone, so that the oracle itself has no gap below NEAR_TIE there
(smallest gaps: 2.6e-3 plain, 4.6e-2 with bias / penalty / min_new_tokens): the exemption never decides the test."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mgea import synth
from test_repetition_penalty_host import penalize
from test_token_grammar_host import ENDPOINT_PROMPT, random_grammar

pytestmark = pytest.mark.gpu
NEAR_TIE = 1e-4
NINF = -math.inf
SETTINGS = ((None, None), (50, None), (None, 0.92), (50, 0.92), (1, None))   # (top_k, top_p), as the bias and penalty tests
ORACLE_SEED = {"plain": 112, "full": 112}   # see the module docstring; checked again by the tests (gaps.min() >= NEAR_TIE)


def make(g, max_batch=8, max_ctx=None, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, **kw), sd, n_head


def host_walk(g, start, ids):
    """the state after the ids a row produced (-1 entries: the row had finished)"""
    return g.run([i for i in ids if i >= 0], start)


def ref_grammar_greedy(ref, prompts, n_steps, g, starts, bias=None, eos=None, min_new=None, penalty=None):
    """DecoderRef.forward per step; (penalize,) + bias, the mask of TokenGrammar.allowed(state), the EOS ban while step < min_new,
    argmax (lowest id among equals); the state advances with TokenGrammar.step.  Returns ids [B][n_steps] (-1 after a row's EOS),
    the processed top-2 gap of every (row, step) and the final states."""
    B = len(prompts)
    Tp = max(len(q) for q in prompts)
    idx = torch.zeros(B, Tp, dtype=torch.long)
    valid = torch.zeros(B, Tp, dtype=torch.bool)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
        valid[b, :len(q)] = True
    _, cache, cvalid = ref.forward(idx, None, None, valid)
    last = torch.tensor([q[-1] for q in prompts]).view(B, 1)
    seen = [set(q) for q in prompts]
    state = list(starts)
    out, gaps = [[] for _ in range(B)], np.full((B, n_steps), np.inf)
    done = [False] * B
    for s in range(n_steps):
        logits, cache, cvalid = ref.forward(last, cache, cvalid, None)
        x = logits[:, -1, :].numpy().astype(np.float32)
        if penalty is not None:
            x = penalize(x, seen, penalty)
        if bias is not None:
            x = (x + bias).astype(np.float32)
        for b in range(B):
            if state[b] >= 0 and not done[b]:
                x[b, ~g.allowed(state[b])] = NINF
            if eos is not None and eos[b] >= 0 and min_new is not None and s < min_new[b]:
                x[b, eos[b]] = NINF
        nxt = x.argmax(1)
        srt = np.sort(x, 1)
        with np.errstate(invalid="ignore"):
            gaps[:, s] = np.where(np.isfinite(srt[:, -2]) & ~np.array(done), srt[:, -1] - srt[:, -2], np.inf)
        for b in range(B):
            out[b].append(-1 if done[b] else int(nxt[b]))
            if not done[b]:
                seen[b].add(int(nxt[b]))
                if state[b] >= 0:
                    state[b] = g.step(state[b], int(nxt[b]))
                    assert state[b] >= 0
                done[b] = eos is not None and eos[b] >= 0 and int(nxt[b]) == eos[b]
        last = torch.from_numpy(nxt.astype(np.int64)).view(B, 1)
    return out, gaps, state


def exempted_rows(got, want, gaps, label):
    n = 0
    for b, (a, w) in enumerate(zip(got, want)):
        if a != w:
            s = next(i for i in range(len(w)) if a[i] != w[i])
            assert gaps[b, s] < NEAR_TIE, f"{label}: row {b} diverged at step {s} (processed top-2 gap {gaps[b, s]:.3e})"
            print(f"[grammar] {label}: row {b} differs at step {s} on a near-tie ({gaps[b, s]:.3e})")
            n += 1
    return n


def oracle_case(golden, kind):
    """decoder_tiny, B = 3 ragged prompts, a 4-state random grammar over 7 classes, rows in different states"""
    g = golden("decoder_tiny")
    V = int(g["cfg"][1])
    rng = np.random.default_rng(ORACLE_SEED[kind])
    prompts = [list(rng.integers(0, V, int(rng.integers(4, 13)))) for _ in range(3)]
    gram = random_grammar(rng, V, 4, 7)
    starts = [0, 3, 1]
    bias = (rng.standard_normal((3, V)) * 2).astype(np.float32)
    return g, prompts, gram, starts, bias


# ---------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("n_class", [1, 33, 4096])
@pytest.mark.parametrize("V", [100, 8324, 14336])
def test_op_sample_grammar_vs_restatement(V, n_class):
    from mgea import ops
    from mgea.decoder import RowSampling
    from oracle.decoder_ref import DecoderRef
    rng = np.random.default_rng(2000 + V + n_class)
    B, n_state = 4, 8 if n_class == 4096 else 3
    g = random_grammar(rng, V, n_state, n_class)
    states = [0, n_state - 1, 1, -1]
    logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32))
    dev = logits.cuda()
    bias_m = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    bias_m[rng.random((B, V)) < 0.3] = NINF
    mask_m = rng.random((B, V)) < 0.2
    allowed = np.stack([g.allowed(s) if s >= 0 else np.ones(V, bool) for s in states])
    for bias, mask, pen in ((None, None, None), (bias_m, mask_m, 1.3)):
        x = logits.numpy() if pen is None else penalize(logits.numpy(), mask, pen)
        x = (x if bias is None else (x + bias)).astype(np.float32)
        x[~allowed] = NINF
        x = torch.from_numpy(x)
        assert bool(torch.isfinite(x).any(dim=1).all())
        pres = None if mask is None else torch.from_numpy(mask)
        for temp in (1.0, 0.7):
            for k, tp in SETTINGS:
                label = f"V={V} n_class={n_class} bias={bias is not None} T={temp} k={k} top_p={tp}"
                rows = [RowSampling(temp, k, tp, pen, seed=9, logit_bias=None if bias is None else bias[b]) for b in range(B)]
                want = DecoderRef.masked_probs(x, temp, min(k, V) if k else None, tp)
                assert bool(torch.isfinite(want).all()) and bool((want[torch.isinf(x)] == 0).all()), label
                ids, s_out, probs = ops.sample_rows_grammar(dev, rows, g, states, step=3, want_probs=True, presence=pres)
                np.testing.assert_allclose(probs.cpu().numpy(), want.numpy(), atol=2e-6, rtol=1e-4, err_msg=label)
                got = ids.cpu().tolist()
                assert bool((want.gather(1, ids.cpu().long()[:, None]) > 0).all()), label + ": drew outside the kept set"
                assert all(allowed[b, got[b]] for b in range(B)), label + ": drew an id its state bans"
                if k == 1:
                    assert got == x.numpy().argmax(1).tolist(), label
                assert s_out.cpu().tolist() == [g.step(s, i) if s >= 0 else -1 for s, i in zip(states, got)], label
                # the row at -1 computes what the op without a grammar computes, to the bit
                o_ids, o_probs = ops.sample_rows(dev, rows, step=3, want_probs=True, presence=pres)
                assert int(o_ids[3]) == got[3] and torch.equal(o_probs[3], probs[3]), label + ": the unconstrained row changed"


# ---------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_one_state_grammar_equals_its_static_bias(golden, tag):
    """fused tail (decoder_tiny8h) and unfused (decoder_tiny); 20 steps = two 8-step graphs and four single steps"""
    from mgea.decoder import RowSampling, TokenGrammar
    g = golden("decoder_" + tag)
    eng, _, _ = make(g, max_batch=4)
    V = eng.vocab
    prompts = [g["prompt0"].tolist(), g["prompt1"].tolist()]
    assert len(prompts[0]) != len(prompts[1])
    rng = np.random.default_rng(17)
    banned = rng.random(V) < 0.5
    gram = TokenGrammar(banned.astype(np.int32), np.array([[0, -1]], np.int32))
    bias = np.where(banned, NINF, 0.0).astype(np.float32)
    eng.set_grammar(gram)
    assert eng.grammar_info() == dict(n_state=1, n_class=2, uploads=1, grammar_steps=0)
    for k, pen in ((20, None), (1, None), (20, 1.2)):
        with_bias = eng.generate_rows(prompts, [RowSampling(1.0, k, None, pen, seed=7, logit_bias=bias) for _ in prompts], 20).cpu()
        assert eng.stats()["biased_steps"] == 20 and eng.grammar_info()["grammar_steps"] == 0
        with_gram = eng.generate_rows(prompts, [RowSampling(1.0, k, None, pen, seed=7, grammar_state=0) for _ in prompts], 20).cpu()
        assert eng.grammar_info()["grammar_steps"] == 20 and eng.stats()["biased_steps"] == 0
        assert torch.equal(with_bias, with_gram), f"{tag} top_k={k} penalty={pen}"
        assert int(with_gram.min()) >= 0 and not banned[with_gram.numpy()].any()
        assert eng.grammar_states().cpu().tolist() == [0, 0]
    eng.close()


def test_stateful_greedy_vs_oracle(golden):
    from mgea.decoder import RowSampling
    from oracle.decoder_ref import DecoderRef
    g, prompts, gram, starts, _ = oracle_case(golden, "plain")
    eng, sd, n_head = make(g, max_batch=4)
    ref = DecoderRef(sd, n_head)
    eng.set_grammar(gram)
    n = 40
    got = eng.generate_rows(prompts, [RowSampling(1.0, 1, grammar_state=s) for s in starts], n).cpu().tolist()
    want, gaps, final = ref_grammar_greedy(ref, prompts, n, gram, starts)
    print(f"[grammar] plain: min processed top-2 gap {gaps.min():.3e}")
    assert gaps.min() >= NEAR_TIE, "the seed was chosen so that the oracle has no near-tie"
    assert exempted_rows(got, want, gaps, "plain") <= 1
    for b in range(3):
        assert gram.accepts(got[b], starts[b])
    assert eng.grammar_states().cpu().tolist() == [host_walk(gram, s, r) for s, r in zip(starts, got)] == final
    free = eng.generate_rows(prompts, [RowSampling(1.0, 1) for _ in starts], n).cpu().tolist()
    assert free != got, "the grammar never changed the generation"
    eng.close()


def test_stateful_greedy_with_bias_penalty_and_min_new_vs_oracle(golden):
    from mgea.decoder import RowSampling
    from oracle.decoder_ref import DecoderRef
    g, prompts, gram, starts, bias = oracle_case(golden, "full")
    eng, sd, n_head = make(g, max_batch=4)
    ref = DecoderRef(sd, n_head)
    eng.set_grammar(gram)
    n = 40
    # row b's EOS: the id the oracle draws at its step 8 when nothing stops it
    probe, _, _ = ref_grammar_greedy(ref, prompts, n, gram, starts, bias, penalty=1.2)
    eos = [row[8] for row in probe]
    rows = [RowSampling(1.0, 1, None, 1.2, eos_id=eos[b], logit_bias=bias[b], min_new_tokens=5, grammar_state=starts[b]) for b in range(3)]
    got = eng.generate_rows(prompts, rows, n).cpu().tolist()
    want, gaps, final = ref_grammar_greedy(ref, prompts, n, gram, starts, bias, eos, [5] * 3, 1.2)
    print(f"[grammar] full: min processed top-2 gap {gaps.min():.3e}; produced {[sum(i >= 0 for i in r) for r in want]}")
    assert gaps.min() >= NEAR_TIE, "the seed was chosen so that the oracle has no near-tie"
    assert exempted_rows(got, want, gaps, "bias + penalty + min_new") <= 1
    assert any(-1 in r for r in want), "no row reached its EOS"
    for b in range(3):
        produced = [i for i in got[b] if i >= 0]
        assert gram.accepts(produced, starts[b]) and len(produced) >= 5 and eos[b] not in produced[:5]
    assert eng.grammar_states().cpu().tolist() == [host_walk(gram, s, r) for s, r in zip(starts, got)] == final
    assert eng.grammar_info()["grammar_steps"] > 0 and eng.stats()["biased_steps"] > 0 and eng.stats()["penalized_steps"] > 0
    eng.close()


def track_case(eng):
    from generate_music.grammar import OPEN, start_state, track_grammar
    tok2id = synth.decoder_vocab(eng.vocab, with_eos=True)
    gram = track_grammar(tok2id)
    prompt = [tok2id[t] for t in ENDPOINT_PROMPT]
    assert start_state(gram, prompt) == OPEN
    return tok2id, gram, prompt, OPEN


def test_sampled_generations_hold_the_track_grammar(golden):
    from generate_music.midi import tokens_to_instruments
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=8, max_ctx=128)
    tok2id, gram, prompt, OPEN = track_case(eng)
    names = list(tok2id)
    eng.set_grammar(gram)
    eos = tok2id["[END_SEQUENCE]"]
    prompts = [prompt[:3 + b % 3] + prompt[3:4] for b in range(8)]   # ragged; every one ends on an instrument
    row = lambda b, st: RowSampling(1.0, 0, 0.92, 1.1, eos_id=eos, seed=100 + b, stream=0, grammar_state=st)
    free = eng.generate_rows(prompts, [row(b, None) for b in range(8)], 50).cpu().tolist()
    assert eng.grammar_info()["grammar_steps"] == 0
    assert not all(gram.accepts([i for i in r if i >= 0], OPEN) for r in free), "the model follows the grammar unasked"
    got = eng.generate_rows(prompts, [row(b, None if b == 5 else OPEN) for b in range(8)], 50).cpu().tolist()
    assert eng.grammar_info()["grammar_steps"] > 0
    states = eng.grammar_states().cpu().tolist()
    for b in range(8):
        produced = [i for i in got[b] if i >= 0]
        if b == 5:
            assert got[b] == free[b] and states[b] == -1, "the unconstrained row changed"
            continue
        assert gram.accepts(produced, OPEN), f"row {b} left the grammar"
        assert states[b] == gram.run(produced, OPEN)
        tracks = tokens_to_instruments([names[i] for i in prompts[b] + produced])
        n_named = sum(names[i].startswith("[INSTRUMENT]") for i in prompts[b])   # the prompt's own instrument tokens
        assert sum(len(t.notes) for t in tracks) + len(tracks) - n_named == sum(i != eos for i in produced)   # nothing is dropped
        assert all(len(t.notes) >= 1 for t in tracks[n_named - 1:-1])   # (the last track may have been cut by the 50 steps)
        for t in tracks:
            st = [n.start for n in t.notes]
            assert st == sorted(st)
    assert len({tuple(r) for r in got}) > 1
    eng.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_grammar_graphs_equal_eager_launches_and_are_reused(golden, tune, tag):
    import test_gpu_step_forms as forms
    from mgea import _lib
    from mgea.decoder import RowSampling, TokenGrammar
    g, prompts, bias = forms.case(golden, tag)
    V = int(g["cfg"][1])
    rng = np.random.default_rng(23)
    gram, other = random_grammar(rng, V, 4, 7), random_grammar(rng, V, 4, 7)
    per = 2 if _lib.tune_get("decoder_graph_steps") > 1 else 1

    def run(eng, starts, scored=False):
        rows = [RowSampling(1.0, 20, None, 1.2, forms.EOS, 0, 7, None, bias, 3, s) for s in starts]
        if scored:
            return eng.generate_scored(prompts, rows, forms.N_STEPS).ids.cpu()
        return eng.generate_rows(prompts, rows, forms.N_STEPS).cpu()

    eng, _, _ = make(g, max_batch=4)
    eng.set_grammar(gram)
    a = run(eng, [0, 2])
    assert eng.stats()["graph_instantiates"] == per and eng.stats()["graph_nodes"] > 0
    b = run(eng, [3, None])                       # other start states, one row unconstrained
    eng.set_grammar(other)                        # another table of the same shape
    c = run(eng, [0, 2])
    assert eng.stats()["graph_instantiates"] == per and eng.grammar_info()["uploads"] == 2
    s = run(eng, [0, 2], scored=True)             # "scored" is part of the key, as for the other forms
    assert eng.stats()["graph_instantiates"] == 2 * per and torch.equal(s, c)
    for f in forms.FORMS:                         # the four old forms instantiate what they do without a grammar form around
        forms.run_form(eng, f, prompts, bias)
    assert eng.stats()["graph_instantiates"] == 6 * per and eng.stats()["graphs_cached"] == 6 * per
    run(eng, [1, 1])
    assert eng.stats()["graph_instantiates"] == 6 * per
    eng.set_grammar(random_grammar(rng, V, 5, 7))   # another shape: the grammar form's graphs go, the others stay
    assert eng.stats()["graphs_cached"] == 4 * per
    eng.close()
    tune("decoder_nograph", 1)   # latched when an engine is created
    eager, _, _ = make(g, max_batch=4)
    eager.set_grammar(gram)
    assert torch.equal(run(eager, [0, 2]), a) and torch.equal(run(eager, [3, None]), b)
    eager.set_grammar(other)
    assert torch.equal(run(eager, [0, 2]), c) and torch.equal(run(eager, [0, 2], scored=True), c)
    assert eager.stats()["graph_instantiates"] == 0
    for out, starts, gr in ((a, [0, 2], gram), (b, [3, None], gram), (c, [0, 2], other)):
        for r, st in zip(out.tolist(), starts):
            assert st is None or gr.accepts([i for i in r if i >= 0], st)
    eager.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_forced_ids_advance_the_state_and_a_banned_one_is_flagged(golden, tag):
    from mgea.decoder import ERR_GRAMMAR_BANNED, RowSampling
    g = golden("decoder_" + tag)
    eng, _, _ = make(g, max_batch=4)
    V = eng.vocab
    rng = np.random.default_rng(29)
    gram = random_grammar(rng, V, 4, 7)
    eng.set_grammar(gram)
    prompts = [g["prompt0"].tolist(), g["prompt1"].tolist()]
    starts, n = [0, 2], 10
    forced = []
    for s in starts:   # an admissible continuation per row, drawn on the host
        row = []
        for _ in range(n):
            row.append(int(rng.choice(np.flatnonzero(gram.allowed(s)))))
            s = gram.step(s, row[-1])
        forced.append(row)
    rows = [RowSampling(1.0, 0, seed=3, grammar_state=s) for s in starts]   # no top-k, no top-p: every admissible id is kept
    res = eng.generate_scored(prompts, rows, n, force_ids=forced)
    assert np.isfinite(res.choice_logprobs.cpu().numpy()).all()
    assert res.ids.cpu().tolist() == forced
    assert eng.grammar_states().cpu().tolist() == [gram.run(f, s) for f, s in zip(forced, starts)]
    assert eng.id_errors(raise_error=False) == 0
    # row 0, step 4: an id its state bans there
    s4 = gram.run(forced[0][:4], starts[0])
    bad = int(np.flatnonzero(~gram.allowed(s4))[0])
    broken = [list(forced[0][:4]) + [bad], forced[1]]          # row 0 is free again from step 5 on
    res = eng.generate_scored(prompts, rows, n, force_ids=broken)
    ids, ch = res.ids.cpu().tolist(), res.choice_logprobs.cpu().numpy()
    assert ids[0][:5] == broken[0] and ids[1] == forced[1]
    assert ch[0, 4] == NINF and np.isfinite(np.delete(ch[0], 4)).all() and np.isfinite(ch[1]).all()
    assert np.isfinite(res.logprobs.cpu().numpy()).all()
    # the state stayed at s4 through the banned id: the free steps after it are drawn under s4's rules
    assert gram.accepts(ids[0][5:], s4)
    assert eng.grammar_states().cpu().tolist() == [gram.run(ids[0][5:], s4), gram.run(forced[1], starts[1])]
    assert eng.id_errors(raise_error=False) == ERR_GRAMMAR_BANNED
    assert eng.id_errors(raise_error=False) == 0, "reading the flags clears them"
    eng.close()


def test_fp16_engine_holds_the_grammar(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_tiny8h")
    eng, _, _ = make(g, max_batch=4, dtype="f16")
    gram = random_grammar(np.random.default_rng(31), eng.vocab, 4, 7)
    eng.set_grammar(gram)
    prompts = [g["prompt0"].tolist(), g["prompt1"].tolist(), g["prompt0"].tolist()[:3]]
    starts = [1, 3, 0]
    got = eng.generate_rows(prompts, [RowSampling(0.9, 0, 0.92, 1.1, seed=5, grammar_state=s) for s in starts], 30).cpu().tolist()
    for r, s in zip(got, starts):
        assert min(r) >= 0 and gram.accepts(r, s)
    assert eng.grammar_states().cpu().tolist() == [gram.run(r, s) for r, s in zip(got, starts)]
    eng.close()


def test_errors_name_the_offender(golden):
    from mgea import _lib
    from mgea.decoder import RowSampling, TokenGrammar
    g = golden("decoder_tiny")
    eng, _, _ = make(g, max_batch=4)
    V = eng.vocab
    prompts = [g["prompt0"].tolist(), g["prompt1"].tolist()]
    with pytest.raises(ValueError, match="row 1: grammar_state 0 but no grammar is set"):
        eng.generate_rows(prompts, [RowSampling(), RowSampling(grammar_state=0)], 4)
    gram = random_grammar(np.random.default_rng(37), V, 4, 7)
    eng.set_grammar(gram)
    with pytest.raises(ValueError, match=r"row 0: grammar_state 4 outside \[0, 4\)"):
        eng.generate_rows(prompts, [RowSampling(grammar_state=4), RowSampling()], 4)
    with pytest.raises(ValueError, match="row 1: grammar_state -2"):
        eng.generate_scored(prompts, [RowSampling(), RowSampling(grammar_state=-2)], 4)
    for bad, what in ((TokenGrammar(np.zeros(V, np.int32), np.zeros((4097, 1), np.int32)), "n_state 4097"),
                      (TokenGrammar(np.zeros(V, np.int32), np.zeros((1, 4097), np.int32)), "n_class 4097"),
                      (TokenGrammar(np.zeros(V, np.int32), np.zeros((2048, 513), np.int32)), "cells"),
                      (TokenGrammar(np.zeros(V + 1, np.int32), np.zeros((1, 1), np.int32)), "class_of must be"),
                      (TokenGrammar(np.zeros(V, np.int32), np.full((2, 1), -1, np.int32)), "state 0 admits no class")):
        with pytest.raises(ValueError, match=what):
            eng.set_grammar(bad)
    assert eng.grammar is gram and eng.grammar_info()["uploads"] == 1
    # the native calls refuse the same things by themselves: MGEA_EINVAL and a message that names the offender
    lib, h, sp = eng.lib, eng.h, eng._sp()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.c_void_p)
    keep = [np.zeros(V, np.int32), np.zeros((1, 4097), np.int32), np.full(V, 3, np.int32), np.array([[0, 5]], np.int32),
            np.array([[0, -1], [-1, -1]], np.int32), np.zeros((4097, 1), np.int32)]
    for cls, nxt, S, K, what in ((keep[0], keep[1], 1, 4097, "n_class 4097"), (keep[0], keep[5], 4097, 1, "n_state 4097"),
                                 (keep[0], keep[1], 2048, 513, "exceeds"), (keep[2], keep[3], 1, 2, "class_of[0] = 3"),
                                 (keep[0], keep[3], 1, 2, "next[0][1] = 5"), (keep[0], keep[4], 2, 2, "state 1 admits no class")):
        assert lib.mgea_decoder_set_grammar(h, i32(cls), i32(nxt), S, K, sp) == _lib.EINVAL
        assert what in _lib.last_error(), _lib.last_error()
    assert eng.grammar_info() == dict(n_state=4, n_class=7, uploads=1, grammar_steps=0)
    ids = torch.tensor([p[:3] for p in prompts], dtype=torch.int32, device="cuda")
    out = torch.empty(2, 4, dtype=torch.int32, device="cuda")
    recs = (_lib.RowSampler * 2)(*[RowSampling().record(b) for b in range(2)])
    call = lambda st: lib.mgea_decoder_generate_rows_grammar(h, _lib.ptr(ids), None, 2, 3, 4, recs, None, (C.c_int32 * 2)(*st), None,
                                                             _lib.ptr(out), None, None, sp)
    torch.cuda.synchronize()
    assert call([0, 4]) == _lib.EINVAL and "row 1: start state 4 outside [0, 4)" in _lib.last_error()
    assert call([-1, -1]) == 0 and eng.grammar_info()["grammar_steps"] == 0       # every state -1: the biased call
    assert call([2, -1]) == 0 and eng.grammar_info()["grammar_steps"] == 4
    assert lib.mgea_decoder_set_grammar(h, None, None, 0, 0, sp) == 0 and eng.grammar_info()["n_state"] == 0
    assert call([2, -1]) == _lib.EINVAL and "no grammar is set" in _lib.last_error()
    torch.cuda.synchronize()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- end to end
def test_grammar_endpoints_end_to_end(golden):
    """the constrained endpoint under the track grammar (create_grammar_app: create_constrained_app's parameter list is pinned by
    tests/test_logit_bias_host.py) and the batched one, composed with constrain="scale" """
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_batched_app, create_constrained_app, create_grammar_app
    from emotion_analysis import inference
    from generate_music.grammar import OPEN, start_state, track_grammar
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer

    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=8, max_ctx=256)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))
    gram = track_grammar(gen.tok2id)

    def check(app):
        client = TestClient(app)
        seen = []
        app.state.on_tokens = seen.append
        kw = {"data": {"prompt": "i love life"}} if app.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
        r = client.post("/generate", **kw)
        assert r.status_code == 200 and r.headers["content-type"].startswith("audio/midi") and r.content[:4] == b"MThd"
        assert r.headers["X-Grammar"] == "tracks"
        assert model.engine.grammar_info()["grammar_steps"] > 0
        n_prompt = int(r.headers["X-Prompt-Tokens"])
        ids = [gen.tok2id[t] for t in seen[-1]]
        assert start_state(gram, ids[:n_prompt]) == OPEN
        assert len(ids) > n_prompt and gram.accepts(ids[n_prompt:], OPEN)
        return r

    check(create_grammar_app(model, seq_len=64, temperature=1.0, top_k=0, top_p=0.92, repetition_penalty=1.1))
    r = check(create_grammar_app(model, seq_len=64, temperature=1.0, top_k=50, constrain="scale", min_new_tokens=12, grammar="tracks"))
    assert r.headers["X-Constraint"] == "scale" and model.engine.stats()["biased_steps"] > 0
    app = create_batched_app(model, seq_len=64, temperature=1.0, top_k=50, grammar="tracks")
    try:
        assert check(app).headers["X-Batch-Rows"] == "1"
    finally:
        app.state.batcher.close()
    plain = create_constrained_app(model, seq_len=64, temperature=1.0, top_k=50, constrain="notes")
    client = TestClient(plain)
    kw = {"data": {"prompt": "i love life"}} if plain.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and "X-Grammar" not in r.headers and model.engine.grammar_info()["grammar_steps"] == 0
    with pytest.raises(ValueError, match="grammar must be one of"):
        create_grammar_app(model, seq_len=64, grammar="bars")
