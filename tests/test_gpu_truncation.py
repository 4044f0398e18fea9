"""min-p, typical-p, epsilon and eta cutoff in the HIP sampler on the MI355X (include/mgea.h, mgea_row_truncation): the truncating
sampler against the float64 restatement of tests/truncation_util.py on robust rows, the band and the degenerate rows, the scored and
the grammar forms, a truncated generation replayed step by step, every launch form, graph reuse, the untruncated paths left as they
were, the compositions with guidance and the KV window, the fp16 engine and the drop-in surface.

Probabilities are held to the tolerance of tests/test_gpu_logit_bias.py::test_op_sample_biased_vs_restatement (atol 2e-6 / rtol 1e-4);
kept sets are compared exactly, on rows robust() admits."""
import math
import random

import numpy as np
import pytest
import torch

import truncation_util as tu
from mgea import synth
from test_repetition_penalty_host import penalize

pytestmark = pytest.mark.gpu
NINF = -math.inf
ATOL, RTOL = 2e-6, 1e-4


def make(g, max_batch=8, max_ctx=None, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, **kw)


def rand_prompts(rng, B, vocab, lo, hi):
    return [[int(v) for v in rng.integers(0, vocab, int(rng.integers(lo, hi + 1)))] for _ in range(B)]


def trunc(st):
    from mgea.decoder import Truncation
    return None if st is None else Truncation(**st)


# ---------------------------------------------------------------------------------------------------------- 1. the op
@pytest.mark.parametrize("V", [97, 8324, 14336])
@pytest.mark.parametrize("case", list(tu.CASES))
def test_op_vs_restatement(V, case):
    """each stage alone and all four: plain, and behind top-k 50, top-p 0.9, a penalty and a bias with bans"""
    from mgea import ops
    from mgea.decoder import RowSampling
    st = tu.CASES[case]
    B = 8
    rng = np.random.default_rng(7000 + V + 31 * list(tu.CASES).index(case))
    bias = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    bias[rng.random((B, V)) < 0.3] = NINF
    mask = rng.random((B, V)) < 0.2
    for heavy in (False, True):
        temp, k, tp, pen = (0.8, 50, 0.9, 1.3) if heavy else (1.0, 0, None, None)
        label = f"V={V} {case} heavy={heavy}"

        def process(raw):
            return (penalize(raw, mask, pen) + bias).astype(np.float32) if heavy else raw

        raw = tu.draw_robust(rng, B, V, st, process, temperature=temp, top_k=k, top_p=tp)
        want, kept = tu.truncated_probs(process(raw), st, temp, k, tp)
        rows = [RowSampling(temp, k, tp, pen, seed=9, logit_bias=bias[b] if heavy else None, truncation=trunc(st)) for b in range(B)]
        ids, probs = ops.sample_rows_truncated(torch.from_numpy(raw).cuda(), rows, step=3, want_probs=True,
                                               presence=torch.from_numpy(mask) if heavy else None)
        probs, ids = probs.cpu(), ids.cpu().long()
        got_kept = probs > 0
        print(f"[trunc] {label}: kept {kept.sum(1).tolist()}  max |dp| {float((probs.double() - want).abs().max()):.3e}")
        assert torch.equal(got_kept, kept), f"{label}: kept sets differ in rows {torch.nonzero((got_kept != kept).any(1)).view(-1).tolist()}"
        np.testing.assert_allclose(probs.numpy(), want.numpy(), atol=ATOL, rtol=RTOL, err_msg=label)
        assert bool(kept.gather(1, ids[:, None]).all()), label + ": drew outside the kept set"
        # the same launch again: the same ids and bits
        ids2, probs2 = ops.sample_rows_truncated(torch.from_numpy(raw).cuda(), rows, step=3, want_probs=True,
                                                 presence=torch.from_numpy(mask) if heavy else None)
        assert torch.equal(ids2.cpu().long(), ids) and torch.equal(probs2.cpu(), probs), label


# ---------------------------------------------------------------------------------------------------------- 2. band and degenerate rows
def test_band_and_degenerate_rows():
    from mgea import ops
    from mgea.decoder import RowSampling, Truncation
    V = 97
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((5, V)) * 3).astype(np.float32)
    x[0] = 0.0
    x[0, 11] = math.log(0.3 / 0.7 * (V - 1))      # the band row: a spike of mass 0.3 over a flat tail
    only = np.full(V, NINF, np.float32)
    only[5] = 0.0                                 # row 1: one admissible id
    x[2] = 1.25                                   # row 2: equal logits
    every = Truncation(0.02, 0.8, 1e-4, 1e-3)
    rows = [RowSampling(1.0, 0, seed=3, truncation=Truncation(typical_p=0.2)),
            RowSampling(1.0, 0, seed=3, logit_bias=only, truncation=every),
            RowSampling(1.0, 0, seed=3, truncation=Truncation(typical_p=0.5, epsilon_cutoff=0.5)),
            RowSampling(0.9, 50, 0.9, seed=3, truncation=Truncation()),                 # every stage off inside a truncated batch
            RowSampling(0.9, 1, seed=3, truncation=every)]                               # greedy: the settings are ignored
    dev = torch.from_numpy(x).cuda()
    ids, probs = ops.sample_rows_truncated(dev, rows, step=2, want_probs=True)
    ids, probs = ids.cpu().tolist(), probs.cpu()
    assert float(probs[0, 11]) == 0.0 and int((probs[0] > 0).sum()) == V - 1 and ids[0] != 11   # the argmax has probability exactly 0
    np.testing.assert_allclose(probs[0].numpy()[np.arange(V) != 11], 1.0 / (V - 1), rtol=RTOL)
    assert torch.nonzero(probs[1]).view(-1).tolist() == [5] and float(probs[1, 5]) == 1.0 and ids[1] == 5
    # equal logits: every d is equal, the band is the row; then every p = 1 / 97 < 0.5 and the lowest id alone stays
    assert torch.nonzero(probs[2]).view(-1).tolist() == [0] and ids[2] == 0
    import dataclasses
    plain = [dataclasses.replace(r, truncation=None) for r in rows]
    ids_b, probs_b = ops.sample_rows(dev, plain, step=2, want_probs=True)      # a row has a bias: mgea_op_sample_rows_biased
    assert torch.equal(probs[3], probs_b.cpu()[3]) and ids[3] == int(ids_b[3]), "an all-off row must be bitwise the biased op's"
    assert ids[4] == int(x[4].argmax()) and torch.nonzero(probs[4]).view(-1).tolist() == [ids[4]]
    # NULL records: the op it extends
    ids_n, probs_n = ops.sample_rows_truncated(dev, plain, step=2, want_probs=True)
    assert torch.equal(ids_n, ids_b) and torch.equal(probs_n, probs_b)
    with pytest.raises(RuntimeError, match="row 1: typical_p"):
        from mgea import _lib
        recs = (_lib.RowTruncation * 5)()
        recs[1].typical_p = 1.5
        from mgea.decoder import pack_rows
        out = torch.empty(5, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().mgea_op_sample_rows_truncated(_lib.ptr(dev), 5, V, pack_rows(plain, V), None, None, recs, 0, _lib.ptr(out), None,
                                                             None, None, None, None, None, 0, 0, None, None, _lib.stream_ptr()))


# ---------------------------------------------------------------------------------------------------------- 3. scored
def test_scored_choice_and_forced_outside_the_kept_set():
    from mgea import ops
    from mgea.decoder import RowSampling
    V, B = 8324, 4
    st = tu.CASES["all"]
    rng = np.random.default_rng(13)
    raw = tu.draw_robust(rng, B, V, st, temperature=0.9)
    want, kept = tu.truncated_probs(raw, st, 0.9)
    rows = [RowSampling(0.9, 0, seed=21, truncation=trunc(st)) for _ in range(B)]
    dev = torch.from_numpy(raw).cuda()
    ids, lp, ch, probs = ops.sample_rows_truncated(dev, rows, step=5, want_probs=True, scored=True)
    ids, lp, ch, probs = ids.cpu().long(), lp.cpu(), ch.cpu(), probs.cpu()
    assert torch.equal(probs > 0, kept)
    np.testing.assert_allclose(ch.numpy(), np.log(probs.gather(1, ids[:, None]).view(-1).numpy()), atol=1e-5, rtol=1e-5)
    raw_lp = torch.log_softmax(torch.from_numpy(raw).double(), -1).gather(1, ids[:, None]).view(-1)
    np.testing.assert_allclose(lp.numpy(), raw_lp.numpy(), atol=1e-4)
    assert torch.equal(ids, ops.sample_rows_truncated(dev, rows, step=5).cpu().long())          # the unscored form draws the same ids
    # a forced id outside the kept set is taken, its raw log-probability is reported and its choice log-probability is -inf
    outside = [int(torch.nonzero(~kept[b]).view(-1)[0]) for b in range(B)]
    inside = [int(torch.nonzero(kept[b]).view(-1)[0]) for b in range(B)]
    forced = [outside[0], -1, inside[2], outside[3]]
    ids_f, lp_f, ch_f = ops.sample_rows_truncated(dev, rows, step=5, scored=True, forced=forced)
    ids_f, ch_f = ids_f.cpu().tolist(), ch_f.cpu()
    assert ids_f == [outside[0], int(ids[1]), inside[2], outside[3]]
    assert ch_f[0] == NINF and ch_f[3] == NINF and float(ch_f[1]) == float(ch[1])
    assert abs(float(ch_f[2]) - math.log(float(probs[2, inside[2]]))) < 1e-5
    assert bool(torch.isfinite(lp_f.cpu()).all())


# ---------------------------------------------------------------------------------------------------------- 4. grammar + truncation
def test_grammar_mask_first_then_truncation_in_one_call():
    from mgea import ops
    from mgea.decoder import RowSampling, TokenGrammar
    V, B = 8324, 4
    st = tu.CASES["typical_hi"]
    # classes: id % 3; state 0 admits class 0 (-> 1), state 1 admits classes 1 and 2 (-> 0, 1)
    gram = TokenGrammar(np.arange(V, dtype=np.int32) % 3, np.array([[1, -1, -1], [-1, 0, 1]], np.int32))
    states = [0, 1, -1, 1]
    rng = np.random.default_rng(17)

    def process(raw):
        x = raw.copy()
        for b, s in enumerate(states):
            if s >= 0:
                x[b, ~gram.allowed(s)] = NINF
        return x

    raw = tu.draw_robust(rng, B, V, st, process)
    want, kept = tu.truncated_probs(process(raw), st)
    rows = [RowSampling(1.0, 0, seed=5, truncation=trunc(st)) for _ in range(B)]
    dev = torch.from_numpy(raw).cuda()
    ids, s_out, probs = ops.sample_rows_truncated(dev, rows, step=1, want_probs=True, grammar=gram, states=states)
    ids, probs = ids.cpu().tolist(), probs.cpu()
    assert torch.equal(probs > 0, kept)
    np.testing.assert_allclose(probs.numpy(), want.numpy(), atol=ATOL, rtol=RTOL)
    assert s_out.cpu().tolist() == [gram.step(s, i) if s >= 0 else -1 for s, i in zip(states, ids)]
    assert ids[0] % 3 == 0 and ids[1] % 3 != 0 and ids[3] % 3 != 0
    # and scored on top: the same ids, the choice log-probability of the same distribution
    ids2, lp, ch, s2 = ops.sample_rows_truncated(dev, rows, step=1, scored=True, grammar=gram, states=states)
    assert ids2.cpu().tolist() == ids and torch.equal(s2, s_out)
    np.testing.assert_allclose(ch.cpu().numpy(), np.log(probs.numpy()[np.arange(B), ids]), atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------- 5. engine replay
def test_truncated_generation_replayed_through_step(golden):
    from mgea import ops
    from mgea.decoder import RowSampling, Truncation
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    V = eng.vocab
    rng = np.random.default_rng(67)
    prompts = rand_prompts(rng, 4, V, 4, 9)
    B, Tp, n_steps, seed, temp = 4, max(len(q) for q in prompts), 40, 4321, 0.9
    t = Truncation(min_p=0.02, typical_p=0.8)
    idx = torch.zeros(B, Tp, dtype=torch.long)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
    lens = torch.tensor([len(q) for q in prompts])
    rows = [RowSampling(temp, 0, None, 1.2, seed=seed, truncation=t) for _ in range(B)]
    out = eng.generate_rows(prompts, rows, n_steps).cpu()
    assert eng.truncation_info() == {"steps": n_steps, "rows": B}
    assert eng.stats()["penalized_steps"] == n_steps
    plain = eng.generate_rows(prompts, [RowSampling(temp, 0, None, 1.2, seed=seed) for _ in range(B)], n_steps).cpu()
    assert eng.truncation_info() == {"steps": 0, "rows": 0}
    assert not torch.equal(out, plain), "the truncated run must differ from the untruncated one"
    eng.reset_and_prefill(idx, lens, want_logits=False, max_len=Tp + n_steps)
    seen = [set(q) for q in prompts]
    fed = torch.tensor([q[-1] for q in prompts], dtype=torch.int32)
    for s in range(n_steps):
        _, lg = eng.step(fed, eng.sampler(1.0, 1), want_logits=True)
        got = ops.sample_rows_truncated(lg, rows, step=s, presence=[sorted(x) for x in seen]).cpu().tolist()
        assert got == out[:, s].tolist(), f"step {s}: replay {got} vs generate {out[:, s].tolist()}"
        for b in range(B):
            seen[b].add(int(out[b, s]))
        fed = out[:, s].to(torch.int32)


# ---------------------------------------------------------------------------------------------------------- 6. launch forms
def test_launch_forms_agree(golden):
    from mgea import _lib
    from mgea.decoder import RowSampling, Truncation
    g = golden("decoder_S")
    rng = np.random.default_rng(71)
    V = int(g["cfg"][1])
    prompts4 = rand_prompts(rng, 4, V, 5, 9)
    n = 48

    def run(switches, prompts):
        old = {k: _lib.tune_set(k, v) for k, v in switches.items()}   # (the engine switches are latched at create)
        try:
            eng = make(g, max_batch=8)
            rows = [RowSampling(0.9, 0, None, 1.2, seed=5, truncation=Truncation(0.02, 0.8, 1e-4, 1e-3)) for _ in prompts]
            out = eng.generate_rows(prompts, rows, n).cpu()
            assert eng.truncation_info()["steps"] == n
            eng.close()
            return out
        finally:
            for k, v in old.items():
                _lib.tune_set(k, v)

    for prompts in (prompts4, prompts4[:1]):      # B = 4 and the GEMV path of B = 1
        base = run({"decoder_graph_steps": 1}, prompts)
        assert int(base.min()) >= 0
        for sw in ({"decoder_unfused": 1}, {"decoder_nograph": 1}, {"decoder_graph_steps": 8}):
            assert torch.equal(base, run(sw, prompts)), f"B={len(prompts)} {sw}"


# ---------------------------------------------------------------------------------------------------------- 7. graphs and untouched paths
def test_graph_reuse_and_untouched_paths(golden):
    from mgea.decoder import RowSampling, Truncation
    g = golden("decoder_S")
    rng = np.random.default_rng(73)
    V = int(g["cfg"][1])
    prompts = rand_prompts(rng, 4, V, 5, 9)
    eng, fresh = make(g, max_batch=8), make(g, max_batch=8)
    n = 40

    def rows(t, k=50, pen=None, **kw):
        return [RowSampling(0.9, k, None, pen, seed=11 + b, stream=b, truncation=t[b] if isinstance(t, list) else t, **kw) for b in range(4)]

    # two requests with different values replay one graph
    a = eng.generate_rows(prompts, rows(Truncation(min_p=0.05)), n).cpu()
    inst = eng.stats()["graph_instantiates"]
    b = eng.generate_rows(prompts, rows(Truncation(typical_p=0.5, eta_cutoff=1e-3), pen=1.3), n).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "other truncation values must replay the cached graphs"
    assert not torch.equal(a, b)
    assert torch.equal(b, fresh.generate_rows(prompts, rows(Truncation(typical_p=0.5, eta_cutoff=1e-3), pen=1.3), n).cpu())

    # records that are all off: the ids of the same call without records, and nothing new is captured
    for k in (1, 50):
        want = fresh.generate_rows(prompts, rows(None, k), n).cpu()
        nodes, inst_f = fresh.stats()["graph_nodes"], fresh.stats()["graph_instantiates"]
        got = fresh.generate_rows(prompts, rows(Truncation(typical_p=1.0), k), n).cpu()
        assert torch.equal(got, want) and fresh.truncation_info() == {"steps": 0, "rows": 0}
        assert fresh.stats()["graph_nodes"] == nodes and fresh.stats()["graph_instantiates"] == inst_f
    # greedy rows ignore their records: still the greedy head
    want = fresh.generate(prompts, n, 1.0, 1).cpu()
    nodes = fresh.stats()["graph_nodes"]
    got = fresh.generate_rows(prompts, [RowSampling(1.0, 1, truncation=Truncation(min_p=0.5)) for _ in range(4)], n).cpu()
    assert torch.equal(got, want) and fresh.stats()["graph_nodes"] == nodes and fresh.truncation_info()["steps"] == 0
    # ... and the untruncated engine paths are what they were after truncated generations ran on the handle
    assert torch.equal(eng.generate(prompts, n, 1.0, 1).cpu(), want)
    assert torch.equal(eng.generate(prompts, n, 0.9, 50, seed=2).cpu(), fresh.generate(prompts, n, 0.9, 50, seed=2).cpu())

    # a mixed batch: rows without settings keep the ids they get in a biased-form batch of that size
    for k, pen in ((50, None), (0, 1.3)):
        base = eng.generate_rows(prompts, rows(None, k, pen, min_new_tokens=n, eos_id=3), n).cpu()     # min_new_tokens: the BIASED form
        assert eng.stats()["biased_steps"] == n
        mixed = eng.generate_rows(prompts, rows([Truncation(typical_p=0.3), None, Truncation(), Truncation(min_p=0.3)], k, pen,
                                                min_new_tokens=n, eos_id=3), n).cpu()
        assert eng.truncation_info() == {"steps": n, "rows": 2}
        assert torch.equal(mixed[1], base[1]) and torch.equal(mixed[2], base[2]), f"top_k={k} penalty={pen}"
        assert not torch.equal(mixed[0], base[0]) and not torch.equal(mixed[3], base[3])


# ---------------------------------------------------------------------------------------------------------- 8. compositions
def test_guided_pair_and_windowed_run_with_min_p(golden):
    from mgea.decoder import RowSampling, Truncation
    g = golden("decoder_S")
    V = int(g["cfg"][1])
    rng = np.random.default_rng(79)
    prompts = rand_prompts(rng, 2, V, 6, 9)
    eng = make(g, max_batch=8)
    rows = [RowSampling(0.9, 0, seed=4 + b, truncation=Truncation(min_p=0.05)) for b in range(2)]
    out = eng.generate_guided(prompts, [prompts[0][:3], None], rows, 1.5, 24, all_rows=True).cpu()
    assert out.shape == (3, 24) and int(out.min()) >= 0 and int(out.max()) < V
    assert torch.equal(out[2], out[0]), "the shadow row ends with its partner's ids"
    assert eng.truncation_info()["steps"] == 24 and eng.guidance_info()["pairs"] == 1
    eng.close()
    # a windowed run past max_ctx
    win = make(g, max_batch=4, max_ctx=192)
    win.set_window(1, None, max_steps=300)
    out = win.generate_rows(prompts, rows, 260).cpu()
    assert out.shape == (2, 260) and int(out.min()) >= 0 and int(out.max()) < V
    assert win.truncation_info()["steps"] == 260 and min(win.window_evictions()) >= 1


# ---------------------------------------------------------------------------------------------------------- 9. f16 engine
def test_f16_engine_typical_p_is_deterministic():
    from mgea.decoder import DecoderEngine, RowSampling, Truncation
    V, L, C, NL = 8324, 256, 256, 2
    sd = synth.decoder_state_dict(41, V, L, C, NL)
    eng = DecoderEngine(sd, n_head=4, max_batch=8, max_ctx=L, dtype="f16")
    prompts = rand_prompts(np.random.default_rng(83), 8, V, 16, 48)
    rows = [RowSampling(1.0, 0, None, 1.1, seed=3, truncation=Truncation(typical_p=0.9)) for _ in range(8)]
    a = eng.generate_rows(prompts, rows, 64).cpu()
    assert eng.truncation_info() == {"steps": 64, "rows": 8} and eng.stats()["graph_replays"] == 64
    b = eng.generate_rows(prompts, rows, 64).cpu()
    assert torch.equal(a, b) and int(a.min()) >= 0 and int(a.max()) < V


# ---------------------------------------------------------------------------------------------------------- 10. the surface
def test_drop_in_surface(golden):
    import generate_music.generate as gen
    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=8, max_ctx=256)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    names = list(gen.tok2id)
    prompt = ["[START_SEQUENCE]", names[5], names[20], names[34]]
    a = gen.sample_kvcache_truncated(model, prompt, max_len=48, top_k=0, typical_p=0.9, seed=7)
    assert model.engine.truncation_info()["steps"] > 0
    assert a == gen.sample_kvcache_truncated(model, prompt, max_len=48, top_k=0, typical_p=0.9, seed=7)
    assert a == gen.sample_kvcache_grammar(model, prompt, max_len=48, top_k=0, typical_p=0.9, seed=7)
    plain = gen.sample_kvcache(model, prompt, max_len=48, top_k=0, seed=7)
    assert model.engine.truncation_info()["steps"] == 0 and plain != a and plain[:4] == a[:4] == prompt
    assert plain == gen.sample_kvcache_truncated(model, prompt, max_len=48, top_k=0, seed=7)       # no keyword: the call it always was
    assert gen.generate_batch_truncated(model, [prompt], max_len=48, top_k=0, typical_p=0.9, seed=7) == [a]
    # per-prompt values: request 0 as the single call (stream 0 of its seed), request 1 without settings
    outs = gen.generate_requests(model, [prompt, prompt], max_len=48, top_k=0, seed=[7, 7], typical_p=[0.9, None], min_p=[0.01, None])
    assert model.engine.truncation_info()["rows"] == 1 and model.engine.truncation_info()["steps"] > 0
    assert outs[0] != outs[1] and all(o[:4] == prompt for o in outs)
    with pytest.raises(ValueError, match="typical_p"):
        gen.generate_requests(model, [prompt, prompt], max_len=48, typical_p=[0.9])
    with pytest.raises(ValueError, match="row 0: min_p"):
        gen.sample_kvcache_truncated(model, prompt, max_len=48, min_p=1.5)
    model.engine.close()


def test_endpoint_with_min_p(golden):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_truncated_app
    from emotion_analysis import inference
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
    for batched in (False, True):
        app = create_truncated_app(model, seq_len=64, temperature=1.0, top_k=0, top_p=0.92, repetition_penalty=1.1, min_p=0.05,
                                   batch_requests=batched)
        try:
            client = TestClient(app)
            kw = {"data": {"prompt": "i love life"}} if app.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
            random.seed(3)
            r = client.post("/generate", **kw)
            assert r.status_code == 200 and r.headers["content-type"].startswith("audio/midi") and r.content[:4] == b"MThd"
            assert model.engine.truncation_info()["steps"] > 0 and model.engine.truncation_info()["rows"] == 1
        finally:
            if app.state.batcher is not None:
                app.state.batcher.close()
    model.engine.close()
