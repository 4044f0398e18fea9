"""A causal engine (pos_mode="causal") through the rest of the generation machinery: repetition penalty and its presence bitmaps, logit
bias with min_new_tokens, token grammars, guidance pairs, blend groups, class penalties, truncation in a composed sampled run, budgets
and the cap, the graph modes, and the drop-in surface (GPTWithKV(causal=True), load_checkpoint, sample_kvcache, score_sequence).

The oracle is causal_util.walk on CausalRef: every prompt prefilled WITHOUT its last token, that token fed first, then the generated or
forced ids, with the step's processing assembled from the host rules the reference-mode tests of each form use.  test_causal_host.py
qualifies every case on the CPU (causal_util.input_conditions): the oracle's processed top-2 gap is at least 5 x W x 2e-4 at every
(row, step) of every greedy case, W the sum of the absolute mix weights -- so greedy ids are compared EXACTLY, with no near-tie exemption.

Shapes: B = 4 ragged prompts of 1, 2, 5 and 65 tokens (the last crosses a KV page in the prefill; the 5-token prompt's last id occurs
nowhere else in it), 16 steps; geometries `tiny` (unfused) and `fused` of test_gpu_causal_engine.py, f32, one engine per geometry for
the module.  Teacher-forced runs are scored sampled rows (top_k / top_p off, temperature 0.8) with forced ids drawn on the host from the
ids the form admits: the choice log-probability is then a continuous function of the processed logits.

Bounds, all the project's: raw log-probabilities 2 x F32_TOL = 4e-4 (test_scored_generation_equals_score_prefill); choice
log-probabilities the named bound of the form's reference-mode test (test_gpu_logprobs.ORACLE_TOL, 4 x weight x LOGIT_TOL of
test_gpu_guidance / test_gpu_blend, test_gpu_class_penalty.SCORED_BOUND).

Observed maxima on MI355X (tiny / fused), |engine - oracle|:
  penalty   raw 6.6e-7 / 9.0e-7, choice 8.6e-7 / 1.1e-6
  bias      raw 9.3e-7 / 9.1e-7, choice 4.1e-6 / 6.3e-6
  grammar   raw 6.3e-7 / 8.3e-7, choice 1.1e-6 / 1.0e-6
  guided    raw 5.1e-7 / 9.8e-7, choice 1.4e-6 / 9.0e-7 (per unit weight)
  blended   raw 9.3e-7 / 7.9e-7, choice 1.6e-6 / 2.0e-6 (per unit weight)
  cpen      raw 9.6e-7 / 1.0e-6, choice 1.3e-6 / 1.1e-6
  score_sequence vs the oracle 7.3e-7 / 1.0e-6
Every greedy, presence, state, context and bitwise comparison held exactly; this file's 20 tests and test_gpu_causal_engine.py's 30 ran in 5.6 s
together, the slowest (test_penalty[tiny], which builds the module's first engine) in 0.66 s, every other one of this file in 0.2 s or less.
"""
import contextlib
import dataclasses

import numpy as np
import pytest
import torch

import causal_util as U
from mgea import synth
from parity_util import LOGIT_TOL
from test_gpu_causal_engine import F32_TOL, GEO, _sd, reference
from test_gpu_class_penalty import SCORED_BOUND
from test_gpu_logprobs import ORACLE_TOL

pytestmark = pytest.mark.gpu

KINDS = ["tiny", "fused"]
N = U.FORM_STEPS
MAX_CTX = 384
RAW_TOL = 2 * F32_TOL
_cache = {}


def new_engine(kind, **kw):
    from mgea.decoder import DecoderEngine
    kw.setdefault("max_ctx", MAX_CTX)
    return DecoderEngine(_sd(kind), n_head=GEO[kind]["n_head"], max_batch=12, pos_mode="causal", **kw)


def engine(kind):
    """one engine per geometry for the whole module"""
    if kind not in _cache:
        _cache[kind] = new_engine(kind)
    return _cache[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for v in _cache.values():
        v.close()
    _cache.clear()


@contextlib.contextmanager
def installed(eng, form):
    """the form's grammar and class map on the engine, cleared afterwards"""
    try:
        if form.grammar is not None:
            eng.set_grammar(form.grammar)
        if form.class_of is not None:
            eng.set_penalty_classes(form.class_of)
        yield
    finally:
        if form.grammar is not None:
            eng.set_grammar(None)
        if form.class_of is not None:
            eng.set_penalty_classes(None)


def rows_of(form, B, greedy, seed=5, truncation=None, temperature=None):
    from mgea.decoder import ClassPenalty, RowSampling
    t = temperature or (1.0 if greedy else U.FORM_TEMPERATURE)
    return [RowSampling(t, 1 if greedy else None, None, form.penalty, -1 if form.eos is None else form.eos[b], 0, seed, None,
                        None if form.bias is None else form.bias[b], 0 if form.min_new is None else form.min_new[b],
                        grammar_state=None if form.grammar is None else form.starts[b], truncation=truncation,
                        class_penalty=None if form.cpen is None else ClassPenalty(*form.cpen[b])) for b in range(B)]


def run(eng, groups, weights, rows, n, forced=None, scored=False):
    """the engine call of a case: generate_rows / generate_scored, generate_guided for pairs, generate_blended for groups"""
    k = len(groups[0])
    if k == 1:
        prompts = [g[0] for g in groups]
        return eng.generate_scored(prompts, rows, n, force_ids=forced) if scored else eng.generate_rows(prompts, rows, n)
    if k == 2:
        return eng.generate_guided([g[0] for g in groups], [g[1] for g in groups], rows, [w[0] for w in weights], n, force_ids=forced,
                                   scored=scored)
    return eng.generate_blended(groups, [list(w) for w in weights], rows, n, force_ids=forced, scored=scored)


def check_forced(kind, name, choice_tol, raw_tol=RAW_TOL, inside=None):
    """the case's teacher-forced run against the oracle: ids, raw and choice log-probabilities, per unit mix weight.  inside(eng): the
    caller's own reads while the form is still installed.  Returns (forced, the oracle's walk, the engine's result, the engine)."""
    eng = engine(kind)
    groups, weights, form = U.form_case(kind, name)
    forced, want = U.draw_forced(kind, name)
    with installed(eng, form):
        res = run(eng, groups, weights, rows_of(form, len(groups), greedy=False), N, forced, scored=True)
        assert res.ids.cpu().tolist() == forced
        w = np.array([U.mix_weight(x) for x in weights])[:, None]
        d_raw = np.abs(res.logprobs.cpu().double().numpy() - want["logprobs"]) / w
        d_ch = np.abs(res.choice_logprobs.cpu().double().numpy() - want["choice"]) / w
        print(f"[causal forms] {kind} {name}: max |raw logprob - oracle| {d_raw.max():.3e} (bound {raw_tol:.1e}), "
              f"max |choice logprob - oracle| {d_ch.max():.3e} (bound {choice_tol:.1e}), per unit weight")
        assert d_raw.max() <= raw_tol, f"{kind} {name}: raw log-probabilities off the causal oracle by {d_raw.max():.3e}"
        assert d_ch.max() <= choice_tol, f"{kind} {name}: choice log-probabilities off the causal oracle by {d_ch.max():.3e}"
        if inside is not None:
            inside(eng)
    return forced, want, res, eng


def check_greedy(kind, name, inside=None):
    """free-running greedy ids: exactly the host's (test_causal_host.py holds the oracle's gaps above 5 x W x F32_TOL)"""
    eng = engine(kind)
    groups, weights, form = U.form_case(kind, name)
    want = U.walk(reference(kind), groups, weights, N, form)
    with installed(eng, form):
        got = run(eng, groups, weights, rows_of(form, len(groups), greedy=True), N)
        got = got.cpu().tolist()
        for b in range(len(groups)):
            if got[b] != want["ids"][b]:
                s = next(i for i in range(N) if got[b][i] != want["ids"][b][i])
                raise AssertionError(f"{kind} {name}: row {b} (prompt of {len(groups[b][0])}) step {s}: engine {got[b][s]} vs host "
                                     f"{want['ids'][b][s]}, host top-2 gap {want['gaps'][b, s]:.3e}")
        states = eng.grammar_states().cpu().tolist() if form.grammar is not None else None
        if inside is not None:
            inside(eng)
    return want, got, states, eng


# ------------------------------------------------------------------------------------------------------------------ 1. penalty
@pytest.mark.parametrize("kind", KINDS)
def test_penalty(kind):
    """step 0 of the 5-token row forces that row's LAST PROMPT id: it is in the bitmap although the prefill did not cache it"""
    forced, _, _, eng = check_forced(kind, "penalty", ORACLE_TOL)
    groups, _, form = U.form_case(kind, "penalty")
    assert forced[2][0] == groups[2][0][-1]
    pres = eng.presence().cpu().numpy()
    for b, g in enumerate(groups):
        assert set(np.nonzero(pres[b])[0].tolist()) == set(g[0]) | set(forced[b]), f"{kind}: row {b}: presence after the forced run"
    want, got, _, eng = check_greedy(kind, "penalty")
    assert eng.stats()["penalized_steps"] == N
    pres = eng.presence().cpu().numpy()
    for b, g in enumerate(groups):
        assert set(np.nonzero(pres[b])[0].tolist()) == set(g[0]) | set(got[b]), f"{kind}: row {b}: presence after the greedy run"
    # the uniform entry point: the same ids
    assert eng.generate([g[0] for g in groups], N, 1.0, 1, repetition_penalty=form.penalty).cpu().tolist() == want["ids"]
    assert eng.context_lengths().cpu().tolist() == [len(g[0]) - 1 + N for g in groups]


# --------------------------------------------------------------------------------------------------------- 2. bias, min_new_tokens
@pytest.mark.parametrize("kind", KINDS)
def test_bias_and_min_new_tokens(kind):
    """min_new_tokens = 3 counts GENERATED ids: the EOS id is banned at steps 0, 1 and 2 -- its choice log-probability, read from a
    probe run that forces it there, is -inf -- and admitted at step 3, where row 3's biased EOS ends the greedy row"""
    forced, _, _, eng = check_forced(kind, "bias", ORACLE_TOL)
    groups, weights, form = U.form_case(kind, "bias")
    rows = rows_of(form, len(groups), greedy=False)
    soft = dataclasses.replace(form, temperature=U.FORM_TEMPERATURE)
    for s in range(4):
        probe = [f[:s] + [U.FORM_EOS] for f in forced]
        res = eng.generate_scored([g[0] for g in groups], rows, N, force_ids=probe)
        assert bool((res.ids[:, s + 1:] == -1).all()), "a forced eos_id finishes the row"
        ch, lp = res.choice_logprobs[:, s].cpu().double().numpy(), res.logprobs[:, s].cpu().numpy()
        assert res.ids[:, s].cpu().tolist() == [U.FORM_EOS] * len(groups) and np.isfinite(lp).all()
        if s < 3:
            assert np.isneginf(ch).all(), f"{kind}: step {s}: the EOS id is admitted before min_new_tokens ({ch})"
        else:
            want = U.walk(reference(kind), groups, weights, s + 1, soft, probe)
            assert np.isfinite(ch).all(), f"{kind}: step 3: the EOS id is still banned ({ch})"
            assert np.abs(ch - want["choice"][:, s]).max() <= ORACLE_TOL
    want, got, _, _ = check_greedy(kind, "bias")
    assert got[3][3] == U.FORM_EOS and got[3][4:] == [-1] * (N - 4) and U.FORM_EOS not in got[3][:3]
    assert eng.stats()["biased_steps"] > 0


# ------------------------------------------------------------------------------------------------------------------ 3. grammar
@pytest.mark.parametrize("kind", KINDS)
def test_grammar(kind):
    """the even / odd grammar with a start state per row: the walk starts in the START state -- the fed prompt token does not move it"""
    check_forced(kind, "grammar", ORACLE_TOL)
    info = {}
    want, got, states, eng = check_greedy(kind, "grammar", lambda e: info.update(e.grammar_info()))
    _, _, form = U.form_case(kind, "grammar")
    for b, st in enumerate(form.starts):
        assert [i % 2 for i in got[b]] == [(st + s) % 2 for s in range(N)], f"{kind}: row {b} left the walk from its start state"
    assert states == want["states"]
    assert info["grammar_steps"] == N and info["n_state"] == 2


# ------------------------------------------------------------------------------------------------------------- 4. guided pairs
@pytest.mark.parametrize("kind", KINDS)
def test_guided_pairs(kind):
    """negative prompts p[:1]: every shadow row prefills nothing inside a batch that does prefill"""
    from test_gpu_guidance import weight
    groups, weights, _ = U.form_case(kind, "guided")
    bound = 4 * LOGIT_TOL        # x weight(s): check_forced compares per unit weight
    assert all(U.mix_weight(w) == weight(w[0]) for w in weights)
    forced, want, _, eng = check_forced(kind, "guided", bound, bound)
    plain = U.walk(reference(kind), [g[:1] for g in groups], [(1.0,)] * len(groups), N, None, forced)
    power = np.abs(want["logprobs"] - plain["logprobs"]).max(1)
    assert (power[1:] >= 0.118).all(), f"{kind}: guided and conditional log-probabilities differ by only {power}"
    want, got, _, eng = check_greedy(kind, "guided")
    assert eng.guidance_info() == dict(pairs=len(groups), guided_steps=N)
    assert eng.context_lengths().cpu().tolist() == [len(g[0]) - 1 + N for g in groups] + [N] * len(groups)


# ------------------------------------------------------------------------------------------------------------ 5. blended groups
@pytest.mark.parametrize("kind", KINDS)
def test_blended_groups(kind):
    """groups of three: the leader, its first token alone (a member that prefills nothing) and a prompt of the group's own"""
    from test_gpu_blend import POWER_FLOOR
    groups, weights, _ = U.form_case(kind, "blended")
    bound = 4 * LOGIT_TOL        # x W(weights), per unit weight in check_forced
    forced, want, _, eng = check_forced(kind, "blended", bound, bound)
    plain = U.walk(reference(kind), [g[:1] for g in groups], [(1.0,)] * len(groups), N, None, forced)
    power = np.abs(want["logprobs"] - plain["logprobs"]).max(1)
    assert all(power[b] >= POWER_FLOOR[w] for b, w in enumerate(weights))
    want, got, _, eng = check_greedy(kind, "blended")
    assert eng.blend_info() == dict(groups=len(groups), rows=3 * len(groups), blended_steps=N)
    assert eng.context_lengths().cpu().tolist() == [len(g[0]) - 1 + N for g in groups] + [len(m) - 1 + N for g in groups for m in g[1:]]


# ------------------------------------------------------------------------------------------------------------ 6. class penalties
@pytest.mark.parametrize("kind", KINDS)
def test_class_penalties(kind):
    """window 4 over map12's classes: the window at step t holds generated ids only -- step 0 forces another id of the class of the
    row's last prompt id, which a window that counted the fed prompt token would penalise"""
    info = {}
    check_forced(kind, "cpen", SCORED_BOUND, inside=lambda e: info.update(e.class_penalty_info()))
    assert info == dict(n_class=12, rows=4, class_penalized_steps=N)


# --------------------------------------------------------------------------------------------------- 7. truncation, composition
def composed_rows(kind):
    from mgea.decoder import Truncation
    _, _, form = U.form_case(kind, "composed")
    return rows_of(form, 3, greedy=False, seed=4321, truncation=Truncation(min_p=0.02, typical_p=0.8), temperature=0.9)


@pytest.mark.parametrize("kind", KINDS)
def test_composed_sampled_generation_replayed_through_step(kind):
    """penalty, bias, grammar, min_p and typical_p in one sampled generation, replayed step by step: forward(prompt[:-1]), then
    step(fed, want_logits=True) and the truncating sampler op on the step's logits at the same seed, stream and step -- bitwise"""
    from mgea import ops
    eng = engine(kind)
    groups, _, form = U.form_case(kind, "composed")
    prompts = [g[0] for g in groups]
    rows = composed_rows(kind)
    with installed(eng, form):
        out = eng.generate_rows(prompts, rows, N).cpu()
        assert eng.truncation_info() == {"steps": N, "rows": 3} and eng.grammar_info()["grammar_steps"] == N
        assert int(out.min()) >= 0
        B, Tp = len(prompts), max(len(p) for p in prompts)
        idx = torch.zeros(B, Tp - 1, dtype=torch.long)
        for b, p in enumerate(prompts):
            idx[b, :len(p) - 1] = torch.tensor(p[:-1])
        eng.reset_and_prefill(idx, torch.tensor([len(p) - 1 for p in prompts]), want_logits=False, max_len=Tp + N)
        seen, states = [set(p) for p in prompts], list(form.starts)
        fed = torch.tensor([p[-1] for p in prompts], dtype=torch.int32)
        for s in range(N):
            _, lg = eng.step(fed, eng.sampler(1.0, 1), want_logits=True)
            got, st = ops.sample_rows_truncated(lg, rows, step=s, presence=[sorted(x) for x in seen], grammar=form.grammar, states=states)
            assert got.cpu().tolist() == out[:, s].tolist(), f"{kind} step {s}: replay {got.cpu().tolist()} vs generate {out[:, s].tolist()}"
            states = st.cpu().tolist()
            for b in range(B):
                seen[b].add(int(out[b, s]))
            fed = out[:, s].to(torch.int32)
        assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + N for p in prompts]


# ------------------------------------------------------------------------------------------------- 8. budgets, EOS and the cap
@pytest.mark.parametrize("kind", KINDS)
def test_budgets_eos_and_the_cap(kind):
    """test_budgets_past_the_padded_reservation on a causal engine: max_ctx 128, prompts of 4, 6 and 5 tokens, max_new_tokens 128 - len,
    124 steps.  The documented rule (include/mgea.h): reserved = min(Tp + n_steps, max_ctx) = 128, a row produces
    min(max_new, reserved - len) ids and ends with ctx_len = len - 1 + produced -- one slot short of its pages, never parked."""
    from mgea.decoder import RowSampling
    eng = new_engine(kind, max_ctx=128)
    rng = np.random.default_rng(73)
    prompts = [[int(v) for v in rng.integers(0, eng.vocab, k)] for k in (4, 6, 5)]
    n, reserved = 124, min(6 + 124, 128)
    budgets = [128 - len(p) for p in prompts]
    produced = [min(m, reserved - len(p)) for m, p in zip(budgets, prompts)]
    rows = [RowSampling(top_k=1, max_new_tokens=m) for m in budgets]
    out = eng.generate_rows(prompts, rows, n).cpu()
    assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + k for p, k in zip(prompts, produced)] == [127] * 3
    for b, p in enumerate(prompts):
        assert bool((out[b, :produced[b]] >= 0).all()) and bool((out[b, produced[b]:] == -1).all())
        solo = eng.generate([p] * 3, produced[b], 1.0, 1).cpu()     # uncapped: len + produced = 128 <= max_ctx; the same batch size
        assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + produced[b]] * 3
        assert torch.equal(solo[0], out[b, :produced[b]]), f"{kind}: row {b} differs from its uncapped run"
    # an EOS id out of row 1's own output stops that row there and leaves the others alone
    row1 = out[1].tolist()
    k = [i for i in range(produced[1]) if row1[i] not in row1[:i]][-1]     # the last id that row 1 had not produced before
    rows2 = [rows[0], RowSampling(top_k=1, max_new_tokens=budgets[1], eos_id=row1[k]), rows[2]]
    out2 = eng.generate_rows(prompts, rows2, n).cpu()
    assert out2[1].tolist() == row1[:k + 1] + [-1] * (n - k - 1)
    assert torch.equal(out2[0], out[0]) and torch.equal(out2[2], out[2])
    assert eng.context_lengths().cpu().tolist() == [127, len(prompts[1]) - 1 + k + 1, 127]
    eng.close()


# ------------------------------------------------------------------------------------------------------------- 9. graph modes
@pytest.mark.parametrize("kind", KINDS)
def test_graph_modes_agree(kind, tune):
    """the composed sampled form and the guided greedy form under 8-step graphs, 1-step graphs and eager launches: the same ids"""
    seen = {}
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)      # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng = new_engine(kind)
        groups, _, form = U.form_case(kind, "composed")
        with installed(eng, form):
            composed = eng.generate_rows([g[0] for g in groups], composed_rows(kind), N).cpu()
        groups, weights, form = U.form_case(kind, "guided")
        guided = run(eng, groups, weights, rows_of(form, len(groups), greedy=True), N).cpu()
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        eng.close()
        for name, ids in (("composed", composed), ("guided", guided)):
            assert int(ids.min()) >= 0
            if name in seen:
                assert torch.equal(ids, seen[name]), f"{kind}: the {name} ids under {mode} differ from graphs8"
            seen.setdefault(name, ids)
    if kind in _cache:   # and they are what the module's engine gives (test 4 holds those to the oracle)
        groups, weights, form = U.form_case(kind, "guided")
        assert torch.equal(run(_cache[kind], groups, weights, rows_of(form, len(groups), greedy=True), N).cpu(), seen["guided"])


# ----------------------------------------------------------------------------------------------------------- the drop-in surface
@pytest.mark.parametrize("kind", KINDS)
def test_drop_in_surface(kind, tmp_path):
    """GPTWithKV(causal=True) on the synthetic weights: sample_kvcache(top_k=1) gives CausalRef.generate_greedy's tokens, score_sequence
    causal_step_logits' log-softmax (4e-4: one masked prefill against the cached oracle), and a checkpoint written to disk loads
    through load_checkpoint(causal=True) to the same tokens"""
    import generate_music.generate as gen
    g, ref = GEO[kind], reference(kind)
    sd = {k: torch.from_numpy(v) for k, v in _sd(kind).items()}
    vocab = synth.decoder_vocab(g["vocab"])
    gen.set_vocab(vocab)
    m = gen.GPTWithKV(g["vocab"], g["seq_len"], g["d_model"], g["n_head"], g["n_layer"], causal=True)
    assert m.load_state_dict(gen.remap_state_dict(sd)) == "<All keys matched successfully>"
    path = str(tmp_path / "causal.pt")
    torch.save({"model": sd, "vocab": vocab}, path)
    prompts = U.form_prompts(kind, U.FORM_SEEDS[kind, "plain"])
    want = ref.generate_greedy(prompts, N)
    toks = {}
    for b, p in enumerate(prompts):
        toks[b] = gen.sample_kvcache(m, [gen.id2tok[i] for i in p], max_len=len(p) + N, temperature=1.0, top_k=1)
        assert [gen.tok2id[t] for t in toks[b]] == want[b], f"{kind}: prompt of {len(p)}"
    assert m.engine.causal
    worst = 0.0
    for b, p in enumerate(prompts):
        cont = want[b][len(p):]
        lp = gen.score_sequence(m, [gen.id2tok[i] for i in p], [gen.id2tok[i] for i in cont])
        ref_lp = torch.log_softmax(U.causal_step_logits(ref, [p], [cont])[0].double(), 1)[torch.arange(N), torch.tensor(cont)]
        worst = max(worst, float((torch.tensor(lp, dtype=torch.float64) - ref_lp).abs().max()))
    print(f"[causal forms] {kind}: max |score_sequence - oracle| = {worst:.3e}")
    assert worst <= RAW_TOL
    model, tok2id, id2tok, seq_len, d_model = gen.load_checkpoint(path, n_head=g["n_head"], causal=True)
    assert model.causal and (seq_len, d_model) == (g["seq_len"], g["d_model"])
    for b, p in enumerate(prompts):
        assert gen.sample_kvcache(model, [id2tok[i] for i in p], max_len=len(p) + N, temperature=1.0, top_k=1) == toks[b]
