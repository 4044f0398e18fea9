"""Repetition penalty on the MI355X: the PENALTY sampler against the fp32 restatement, penalized greedy generation against the
oracle, the presence bitmaps, the sampled draw replayed step by step, every launch form of generate(), the fp16 engine, the
unpenalized paths left as they were, and the paper's decoding setting end to end."""
import random

import numpy as np
import pytest
import torch

from mgea import synth
from test_repetition_penalty_host import penalize

pytestmark = pytest.mark.gpu
NEAR_TIE = 1e-4


def make(g, max_batch=8, max_ctx=None, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, **kw), sd, n_head


def rand_prompts(rng, B, vocab, lo, hi):
    return [list(rng.integers(0, vocab, int(rng.integers(lo, hi + 1)))) for _ in range(B)]


def ref_penalized_greedy(ref, prompts, n_steps, p):
    """DecoderRef.forward per step, penalize over prompt + generated, argmax (lowest id among equals).  Returns the generated
    ids [B][n_steps] and the penalized top-2 gap of every (row, step)."""
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
    out, gaps = [[] for _ in range(B)], np.zeros((B, n_steps))
    for s in range(n_steps):
        logits, cache, cvalid = ref.forward(last, cache, cvalid, None)
        x = penalize(logits[:, -1, :].numpy(), seen, p)
        nxt = x.argmax(1)
        srt = np.sort(x, 1)
        gaps[:, s] = srt[:, -1] - srt[:, -2]
        for b in range(B):
            out[b].append(int(nxt[b]))
            seen[b].add(int(nxt[b]))
        last = torch.from_numpy(nxt.astype(np.int64)).view(B, 1)
    return out, gaps


def assert_ids_match(got, want, gaps, label):
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            s = next(i for i in range(len(w)) if g[i] != w[i])
            assert gaps[b, s] < NEAR_TIE, f"{label}: row {b} diverged at step {s} (penalized top-2 gap {gaps[b, s]:.3e})"
            print(f"[penalty] {label}: row {b} differs at step {s} on a near-tie ({gaps[b, s]:.3e})")


# ---------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("V", [100, 8324, 14336])
def test_op_sample_penalized_vs_restatement(V):
    from mgea import ops
    from oracle.decoder_ref import DecoderRef
    rng = np.random.default_rng(V)
    B = 4
    logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32))
    masks = {"empty": np.zeros((B, V), bool), "random": rng.random((B, V)) < 0.2, "all": np.ones((B, V), bool)}
    for mname, mask in masks.items():
        for p in (0.8, 1.1, 1.5):
            x = torch.from_numpy(penalize(logits.numpy(), mask, p))
            for temp in (1.0, 0.7):
                for k, tp in ((None, None), (50, None), (None, 0.92), (50, 0.92), (1, None)):
                    ids, probs = ops.sample(logits.cuda(), temp, k, tp, seed=9, step=3, want_probs=True, repetition_penalty=p,
                                            presence=torch.from_numpy(mask))
                    want = DecoderRef.masked_probs(x, temp, min(k, V) if k else None, tp)
                    np.testing.assert_allclose(probs.cpu().numpy(), want.numpy(), atol=2e-6, rtol=1e-4,
                                               err_msg=f"{mname} p={p} T={temp} k={k} top_p={tp}")
                    assert bool((want.gather(1, ids.cpu().long()[:, None]) > 0).all()), "drew outside the kept set"
                    if k == 1:
                        assert ids.cpu().tolist() == x.numpy().argmax(1).tolist()


def test_op_sample_penalized_greedy_exact_ties():
    from mgea import ops
    V = 300
    x = torch.full((3, V), -50.0)
    x[0, 10], x[0, 7] = -1.0, -2.0            # seen -1.0 * 2 == unseen -2.0 at a LOWER id: 7 wins
    x[1, 7], x[1, 10] = -2.0, -1.0            # the same with the ids swapped: 7 (unseen, lower) still wins
    x[2, 200], x[2, 100] = 4.0, 2.0           # seen 4.0 / 2 == unseen 2.0 at a lower id: 100 wins
    seen = [[10], [10], [200]]
    ids = ops.sample(x.cuda(), 1.0, 1, None, seed=1, step=0, repetition_penalty=2.0, presence=seen).cpu().tolist()
    assert ids == [7, 7, 100]
    seen = [[7], [7], [100]]                   # now the lower ids are the penalized ones: the higher id wins
    ids = ops.sample(x.cuda(), 1.0, 1, None, seed=1, step=0, repetition_penalty=2.0, presence=seen).cpu().tolist()
    assert ids == [10, 10, 200]
    # without the penalty these rows have a strict maximum
    assert ops.sample(x.cuda(), 1.0, 1, None).cpu().tolist() == [10, 10, 200]


def test_op_sample_penalized_identity_with_empty_presence():
    from mgea import ops
    rng = np.random.default_rng(3)
    logits = torch.from_numpy((rng.standard_normal((6, 8324)) * 3).astype(np.float32)).cuda()
    for temp, k, tp in ((1.0, 50, None), (0.8, None, 0.92), (1.0, 50, 0.92), (1.3, None, None), (1.0, 1, None)):
        a_ids, a_p = ops.sample(logits, temp, k, tp, seed=42, step=5, want_probs=True)
        b_ids, b_p = ops.sample(logits, temp, k, tp, seed=42, step=5, want_probs=True, repetition_penalty=1.3)
        assert torch.equal(a_ids, b_ids)
        if k != 1:   # (top_k = 1: the penalized form keeps the argmax of the raw row, the unpenalized one that of row / T)
            assert torch.equal(a_p, b_p)


def test_op_sample_penalized_bad_arguments():
    from mgea import ops
    x = torch.zeros(1, 10).cuda()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.sample(x, repetition_penalty=bad)


# ---------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("tag", ["S", "tiny"])
def test_engine_penalized_greedy_vs_oracle(golden, tag):
    from oracle.decoder_ref import DecoderRef
    g = golden("decoder_" + tag)
    eng, sd, n_head = make(g, max_batch=64)
    ref = DecoderRef(sd, n_head)
    V, L = eng.vocab, eng.seq_len
    rng = np.random.default_rng(17)
    n_steps = 130 if L >= 256 else L - 12
    changed = False
    for B, lo, hi in ((1, 8, 8), (4, 3, 10), (64, 4, 12)):
        prompts = rand_prompts(rng, B, V, lo, hi)
        for p in (1.1, 1.5):
            got = eng.generate(prompts, n_steps, 1.0, 1, repetition_penalty=p).cpu().tolist()
            assert eng.stats()["penalized_steps"] == n_steps
            want, gaps = ref_penalized_greedy(ref, prompts, n_steps, p)
            assert_ids_match(got, want, gaps, f"{tag} B={B} p={p}")
            plain = eng.generate(prompts, n_steps, 1.0, 1).cpu().tolist()
            changed = changed or plain != got
    assert changed, "the penalty never changed a greedy generation"


def test_presence_readback_greedy_and_sampled(golden):
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=8)
    V = eng.vocab
    rng = np.random.default_rng(23)
    prompts = rand_prompts(rng, 5, V, 3, 12)        # ragged: padding (id 0) must not enter the sets
    eos = 17
    for kw in (dict(top_k=1), dict(top_k=50, seed=4), dict(top_k=0, top_p=0.92, seed=8)):
        out = eng.generate(prompts, 90, 1.0, eos_id=eos, repetition_penalty=1.1, **kw).cpu()
        pres = eng.presence().cpu().numpy()
        assert pres.shape == (5, V)
        for b, q in enumerate(prompts):
            row = out[b].tolist()
            gen_ids = [i for i in row if i >= 0]
            if eos in gen_ids:
                assert gen_ids[-1] == eos and all(i == -1 for i in row[len(gen_ids):])
            want = set(q) | set(gen_ids)
            assert set(np.nonzero(pres[b])[0].tolist()) == want, f"{kw} row {b}"
    eng.generate(prompts, 4, 1.0, top_k=1)
    with pytest.raises(RuntimeError):     # the last generate applied no penalty
        eng.presence()


def test_sampled_penalized_replay_through_step(golden):
    from mgea import ops
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=8)
    V = eng.vocab
    rng = np.random.default_rng(29)
    prompts = rand_prompts(rng, 4, V, 4, 9)
    B, Tp, n_steps, seed, temp = 4, max(len(q) for q in prompts), 40, 1234, 0.9
    idx = torch.zeros(B, Tp, dtype=torch.long)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
    lens = torch.tensor([len(q) for q in prompts])

    def replay(ids, pen):
        eng.reset_and_prefill(idx, lens, want_logits=False, max_len=Tp + n_steps)
        seen = [set(q) for q in prompts]
        fed = torch.tensor([q[-1] for q in prompts], dtype=torch.int32)
        for s in range(n_steps):
            _, lg = eng.step(fed, eng.sampler(1.0, 1), want_logits=True)
            kw = dict(repetition_penalty=pen, presence=[sorted(x) for x in seen]) if pen else {}
            got = ops.sample(lg, temp, 50, None, seed=seed, step=s, **kw).cpu().tolist()
            assert got == ids[:, s].tolist(), f"penalty {pen}: step {s}: replay {got} vs generate {ids[:, s].tolist()}"
            for b in range(B):
                seen[b].add(int(ids[b, s]))
            fed = ids[:, s].to(torch.int32)

    plain = eng.generate(prompts, n_steps, temp, 50, seed=seed).cpu()
    replay(plain, None)          # precondition: the step API's logits are the graph's
    pen = eng.generate(prompts, n_steps, temp, 50, seed=seed, repetition_penalty=1.3).cpu()
    assert not torch.equal(pen, plain)
    replay(pen, 1.3)


def test_launch_forms_agree(golden):
    from mgea import _lib
    g = golden("decoder_S")
    rng = np.random.default_rng(31)
    V = int(g["cfg"][1])
    prompts4 = rand_prompts(rng, 4, V, 5, 9)
    prompts1 = prompts4[:1]
    n = 70

    def run(switches, prompts, **kw):
        old = {k: _lib.tune_set(k, v) for k, v in switches.items()}   # (the engine switches are latched at create)
        try:
            eng, _, _ = make(g, max_batch=8)
            out = eng.generate(prompts, n, 1.0, **kw).cpu()
            eng.close()
            return out
        finally:
            for k, v in old.items():
                _lib.tune_set(k, v)

    for prompts in (prompts4, prompts1):
        base = run({}, prompts, top_k=1, repetition_penalty=1.2)
        assert torch.equal(base, run({"decoder_unfused": 1}, prompts, top_k=1, repetition_penalty=1.2))
        assert torch.equal(base, run({"decoder_nograph": 1}, prompts, top_k=1, repetition_penalty=1.2))
        if len(prompts) == 1:
            assert torch.equal(base, run({"decoder_nogemv": 1}, prompts, top_k=1, repetition_penalty=1.2))
    a = run({"decoder_graph_steps": 1}, prompts4, top_k=50, seed=5, repetition_penalty=1.2)
    b = run({"decoder_graph_steps": 8}, prompts4, top_k=50, seed=5, repetition_penalty=1.2)
    assert torch.equal(a, b)

    eng, _, _ = make(g, max_batch=8)
    eng.generate(prompts4, n, 1.0, top_k=50, seed=5, repetition_penalty=1.2)
    inst = eng.stats()["graph_instantiates"]
    again = eng.generate(prompts4, n, 0.8, top_k=50, top_p=0.9, seed=77, repetition_penalty=1.7).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "a new penalty / seed must replay the cached graph"
    fresh, _, _ = make(g, max_batch=8)
    assert torch.equal(again, fresh.generate(prompts4, n, 0.8, top_k=50, top_p=0.9, seed=77, repetition_penalty=1.7).cpu())


def test_profile_stride_penalized_matches_graph(golden):
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=8)
    rng = np.random.default_rng(37)
    prompts = rand_prompts(rng, 3, eng.vocab, 4, 8)
    want = eng.generate(prompts, 40, 1.0, 1, repetition_penalty=1.25).cpu()
    eng.profile(7)
    got = eng.generate(prompts, 40, 1.0, 1, repetition_penalty=1.25).cpu()
    eng.profile(0)
    eng.profile_read()
    assert torch.equal(want, got)


def test_f16_engine_penalized_top_p():
    from mgea.decoder import DecoderEngine
    V, L, C, NL = 8324, 2112, 768, 12
    sd = synth.decoder_state_dict(41, V, L, C, NL)
    eng = DecoderEngine(sd, n_head=12, max_batch=8, max_ctx=L, dtype="f16")
    rng = np.random.default_rng(43)
    prompts = rand_prompts(rng, 8, V, 16, 48)
    n = 2048
    a = eng.generate(prompts, n, 1.0, top_k=0, top_p=0.9, seed=3, repetition_penalty=1.1).cpu()
    st = eng.stats()
    assert st["graph_replays"] == n and st["penalized_steps"] == n and st["graph_nodes"] > 0
    pres = eng.presence().cpu().numpy()
    b = eng.generate(prompts, n, 1.0, top_k=0, top_p=0.9, seed=3, repetition_penalty=1.1).cpu()
    assert torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < V
    for r, q in enumerate(prompts):
        assert set(np.nonzero(pres[r])[0].tolist()) == set(q) | set(a[r].tolist())


def test_unpenalized_paths_untouched(golden):
    g = golden("decoder_S")
    rng = np.random.default_rng(47)
    prompts = rand_prompts(rng, 4, int(g["cfg"][1]), 5, 9)
    eng, _, _ = make(g, max_batch=8)
    fresh, _, _ = make(g, max_batch=8)
    want = fresh.generate(prompts, 50, 1.0, 1).cpu()
    nodes = fresh.stats()["graph_nodes"]
    eng.generate(prompts, 50, 1.0, 1, repetition_penalty=1.3)
    eng.generate(prompts, 50, 1.0, 50, seed=2, repetition_penalty=1.3)
    got = eng.generate(prompts, 50, 1.0, 1).cpu()
    assert torch.equal(got, want) and eng.stats()["graph_nodes"] == nodes
    assert eng.stats()["penalized_steps"] == 0
    eng.generate(prompts, 50, 1.0, 1, repetition_penalty=1.0)
    assert eng.stats()["penalized_steps"] == 0
    assert torch.equal(eng.generate(prompts, 50, 1.0, 50, seed=2, repetition_penalty=1.0).cpu(),
                       fresh.generate(prompts, 50, 1.0, 50, seed=2).cpu())
    eng.generate(prompts, 33, 1.0, 1, repetition_penalty=1.3)
    assert eng.stats()["penalized_steps"] == 33


# ---------------------------------------------------------------------------------------------------------- paper setting
def test_paper_setting_end_to_end(golden):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_app
    from emotion_analysis import inference
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer

    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    assert "[END_SEQUENCE]" in gen.tok2id
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=64, max_ctx=256)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    names = list(gen.tok2id)
    prompt = ["[START_SEQUENCE]"] + names[40:46]
    toks = gen.sample_kvcache(model, prompt, 200, 1.0, top_k=0, top_p=0.92, repetition_penalty=1.1, seed=5)
    assert toks[:len(prompt)] == prompt and len(prompt) < len(toks) <= 200
    if "[END_SEQUENCE]" in toks:
        assert toks.index("[END_SEQUENCE]") == len(toks) - 1
    assert model.engine.stats()["penalized_steps"] > 0
    rows = gen.generate_batch(model, [prompt] * 64, 120, 1.0, top_k=0, top_p=0.92, seed=6, repetition_penalty=1.1)
    assert len(rows) == 64 and len({tuple(r) for r in rows}) > 1
    for r in rows:
        assert r[:len(prompt)] == prompt and len(r) <= 120
        if "[END_SEQUENCE]" in r:
            assert r.index("[END_SEQUENCE]") == len(r) - 1

    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))
    app = create_app(model, seq_len=48, temperature=1.0, top_k=0, top_p=0.92, repetition_penalty=1.1)
    client = TestClient(app)
    kw = {"data": {"prompt": "i love life"}} if app.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
    random.seed(3)
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and r.headers["content-type"].startswith("audio/midi") and r.content[:4] == b"MThd"
    assert model.engine.stats()["penalized_steps"] > 0
