"""Classifier-free guidance between paired rows on the MI355X (include/mgea.h, mgea_decoder_generate_rows_guided): the mix kernel
alone against float64, guided generations against the oracle run on both prompts (teacher-forced log-probabilities; free-running
greedy ids against the host's guided maximum), the shadow rows and the step graphs, refusals, a windowed guided run, the endpoint.

Tolerances, per (|s| + |1 - s|) -- the weights of the two rows in g = s logp_c + (1 - s) logp_u:
  op level     OP_TOL = 1e-4 (test_gpu_logprobs: the project's 1e-4 on log-probabilities; plain fp32 is within 2e-6 of float64);
  teacher-forced 4 LOGIT_TOL: each row's log-softmax costs one LOGIT_TOL for the logit and one for the log-sum (2 LOGIT_TOL, weighted
               by |s| and |1 - s|), and the final normalisation of g doubles that;
  greedy       2 x 2 LOGIT_TOL: g at two ids (the chosen one and the host's maximum), each off by at most 2 LOGIT_TOL per unit weight.
"""
import ctypes as C
import functools
import math
import os
import random

import numpy as np
import pytest
import torch

from mgea import synth
from parity_util import LOGIT_TOL
from test_gpu_logprobs import OP_TOL, make
from test_gpu_step_forms import EOS, N_STEPS, case

pytestmark = pytest.mark.gpu
SCALES = (0.0, 1.5, 3.0)
N_FORCED = 12


def weight(s):
    return abs(s) + abs(1.0 - s)


def oracle_logps(ref, prompt, cont):
    """test_gpu_logprobs.oracle_score's loop for one row, keeping the whole float64 log_softmax row of every step: [len(cont), V]"""
    _, cache, valid = ref.forward(torch.tensor([prompt]))
    last = torch.tensor([[prompt[-1]]])
    out = []
    for t in cont:
        logits, cache, valid = ref.forward(last, cache, valid)
        out.append(torch.log_softmax(logits[0, -1].double(), dim=0))
        last = torch.tensor([[t]])
    return torch.stack(out)


def guided_case(vocab):
    """the issue's inputs: default_rng(7); prompts of 3, 6 and 4 random ids, each negative prompt its prompt's first id, 12 forced ids"""
    rng = np.random.default_rng(7)
    prompts = [[int(v) for v in rng.integers(0, vocab, n)] for n in (3, 6, 4)]
    negs = [p[:1] for p in prompts]
    forced = [[int(v) for v in rng.integers(0, vocab, N_FORCED)] for _ in prompts]
    return prompts, negs, forced


def oracle_of(g):
    """the CPU oracle on a golden file's synthetic weights, and its vocabulary size"""
    from oracle.decoder_ref import DecoderRef
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    return DecoderRef(synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer), n_head), vocab


@functools.lru_cache(maxsize=None)
def forced_reference(tag):
    """the teacher-forced oracle rows of guided_case, once per golden: (logp_c, logp_u), each a list of [12, V] float64 per row"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"decoder_{tag}.npz"))
    ref, vocab = oracle_of(g)
    prompts, negs, forced = guided_case(vocab)
    lc = [oracle_logps(ref, p, f) for p, f in zip(prompts, forced)]
    lu = [oracle_logps(ref, q, f) for q, f in zip(negs, forced)]
    return lc, lu


def grammar_of(vocab):
    """two states that alternate between the even and the odd ids"""
    from mgea.decoder import TokenGrammar
    return TokenGrammar(np.arange(vocab) % 2, np.array([[1, -1], [-1, 0]]))


# ------------------------------------------------------------------------------------------------------------ 1. the op alone
@pytest.mark.parametrize("V", [100, 8324, 9217, 14336])   # fewer ids than threads, the real vocabulary, first width past the narrow kernel, the cap
def test_op_guidance_mix(V):
    from mgea import ops
    rng = np.random.default_rng(3000 + V)
    B, partner = 5, [3, -1, -1, -1, 2]
    raw = (rng.standard_normal((B + 1, V)) * 3).astype(np.float32)   # row 5: a guard row behind the buffer the kernel is told about
    x = raw.astype(np.float64)
    logp = x - x.max(axis=1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(axis=1, keepdims=True))     # the reference, once
    dev = torch.from_numpy(raw).cuda()
    worst = 0.0
    for s0, s4 in ((0.0, 1.0), (1.0, 1.5), (1.5, 3.0), (3.0, 0.0)):
        scale = [s0, 7.0, -1.0, math.nan, s4]                         # the scales of rows that are not conditional are not read
        got_t = ops.guidance_mix(dev, partner, scale)
        again = ops.guidance_mix(dev, partner, scale)
        assert torch.equal(got_t, again), f"V={V}: two runs differ"
        got = got_t.cpu().numpy()
        assert torch.equal(dev.cpu(), torch.from_numpy(raw)), "guidance_mix works on a copy"
        for c, u, s in ((0, 3, s0), (4, 2, s4)):
            want = s * logp[c] + (1.0 - s) * logp[u]
            d = float(np.abs(got[c] - want).max())
            worst = max(worst, d / weight(s))
            print(f"[guidance] V={V} s={s}: |g - float64| {d:.2e} (bound {OP_TOL * weight(s):.1e})")
            assert d <= OP_TOL * weight(s), f"V={V} scale {s}: the mixed row is off float64 by {d:.2e}"
            assert got[c].tobytes() == got[u].tobytes(), f"V={V}: rows {c} and {u} differ after the mix"
        assert got[1].tobytes() == raw[1].tobytes(), "an unpaired row was touched"
        assert got[5].tobytes() == raw[5].tobytes(), "the guard row behind the batch was touched"
    print(f"[guidance] V={V}: worst |g - float64| per unit weight {worst:.2e}")
    with pytest.raises(ValueError, match="row 0"):
        ops.guidance_mix(dev, [0, -1, -1, -1, -1], [1.0] * 5)
    with pytest.raises(ValueError, match="row 4"):
        ops.guidance_mix(dev, [3, -1, -1, -1, 3], [1.0] * 5)


# ------------------------------------------------------------------------------------------------- 2. teacher-forced, the oracle
@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])   # unfused / fused tail
def test_guided_logprobs_against_the_oracle(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    eng, _, _ = make(g, max_batch=8)
    prompts, negs, forced = guided_case(eng.vocab)
    lc, lu = forced_reference(tag)
    rows = [RowSampling(top_k=1, eos_id=-1) for _ in prompts]
    steps = torch.arange(N_FORCED)
    for s in SCALES:
        bound = 4 * weight(s) * LOGIT_TOL
        assert bound <= 0.02
        res = eng.generate_guided(prompts, negs, rows, s, N_FORCED, force_ids=forced, scored=True)
        assert res.ids.cpu().tolist() == forced and res.logprobs.shape == (3, N_FORCED)
        assert eng.guidance_info() == dict(pairs=3, guided_steps=N_FORCED)
        for b in range(3):
            ids = torch.tensor(forced[b])
            want = torch.log_softmax(s * lc[b] + (1.0 - s) * lu[b], dim=1)[steps, ids]
            plain = lc[b][steps, ids]
            # power, from the oracle alone: the guided value is far from the plain conditional one at some step, so unmixed logits fail
            power = float((want - plain).abs().max())
            assert power >= 0.118, f"{tag} row {b} scale {s}: guided and conditional log-probabilities differ by only {power:.3f}"
            d = float((res.logprobs[b].cpu().double() - want).abs().max())
            print(f"[guidance] {tag} row {b} scale {s}: |logprob - oracle| {d:.2e} (bound {bound:.1e}; guided vs conditional {power:.3f})")
            assert d <= bound, f"{tag} row {b} scale {s}: guided logprobs off the oracle by {d:.2e} > {bound:.1e}"
    eng.close()


# ------------------------------------------------------------------------------------------------------ 3. greedy, free-running
@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_guided_greedy_ids_are_the_hosts_guided_maximum(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    ref, _ = oracle_of(g)
    eng, _, _ = make(g, max_batch=8)
    prompts, negs, _ = guided_case(eng.vocab)
    rows = [RowSampling(top_k=1, eos_id=-1) for _ in prompts]
    ids = eng.generate_guided(prompts, negs, rows, list(SCALES), N_FORCED).cpu().tolist()
    assert eng.guidance_info() == dict(pairs=3, guided_steps=N_FORCED)
    for b, s in enumerate(SCALES):
        assert len(ids[b]) == N_FORCED and min(ids[b]) >= 0
        gh = s * oracle_logps(ref, prompts[b], ids[b]) + (1.0 - s) * oracle_logps(ref, negs[b], ids[b])   # [12, V]
        top = gh.max(dim=1).values
        at = gh[torch.arange(N_FORCED), torch.tensor(ids[b])]
        gap = float((top - at).max())
        tol = 2 * weight(s) * 2 * LOGIT_TOL
        print(f"[guidance] {tag} row {b} scale {s}: chosen id below the host's guided maximum by at most {gap:.2e} (bound {tol:.1e})")
        assert gap <= tol, f"{tag} row {b} scale {s}: a greedy id is {gap:.2e} below the host's guided maximum"
    eng.close()


# -------------------------------------------------------------------------------------------------- 4. shadow rows and graphs
def row_kinds(vocab, bias):
    from mgea.decoder import RowSampling
    return {"sampled": RowSampling(1.0, 20, seed=7), "penalized": RowSampling(1.0, 20, None, 1.2, seed=7),
            "biased": RowSampling(1.0, 20, None, 1.2, EOS, 0, 7, None, bias, 3),
            "grammar": RowSampling(1.0, 20, None, 1.2, EOS, 0, 7, None, bias, 3, grammar_state=0)}


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_shadow_rows_take_their_conditional_rows_ids_in_every_graph_mode(golden, tune, tag):
    g, prompts, bias = case(golden, tag)
    negs = [p[:1] for p in prompts]
    seen = {}
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng, _, _ = make(g, max_batch=8)
        eng.set_grammar(grammar_of(eng.vocab))
        for kind, row in row_kinds(eng.vocab, bias).items():
            rows = [row for _ in prompts]
            ids = eng.generate_guided(prompts, negs, rows, [1.5, 3.0], N_STEPS, all_rows=True).cpu()
            assert ids.shape == (4, N_STEPS) and eng.guidance_info()["pairs"] == 2
            assert torch.equal(ids[2], ids[0]) and torch.equal(ids[3], ids[1]), f"{tag} {mode} {kind}: a shadow row left its conditional row"
            assert int(ids[:, 0].min()) >= 0
            res = eng.generate_guided(prompts, negs, rows, [1.5, 3.0], N_STEPS, scored=True, all_rows=True)
            assert torch.equal(res.ids.cpu(), ids), f"{tag} {mode} {kind}: scoring changed the guided ids"
            assert torch.equal(res.logprobs[2:], res.logprobs[:2]) and torch.equal(res.choice_logprobs[2:], res.choice_logprobs[:2])
            if kind == "grammar":
                gr = grammar_of(eng.vocab)
                for b in range(2):
                    assert gr.accepts([int(v) for v in ids[b].tolist() if v >= 0]), f"{tag} {mode}: row {b} left the grammar"
                st = eng.grammar_states().cpu().tolist()
                assert st[2:] == st[:2]
            if kind != "sampled":
                pres = eng.presence().cpu()
                assert torch.equal(pres[2], pres[0]) and torch.equal(pres[3], pres[1]), "a pair's penalty set is the conditional row's"
                assert bool(pres[2, prompts[0]].all())
            key = (kind,)
            if key in seen:
                assert torch.equal(ids, seen[key]), f"{tag}: {kind} ids under {mode} differ from graphs8"
            seen.setdefault(key, ids)
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        eng.close()


def test_guided_graphs_are_reused_and_leave_the_unguided_ones_alone(golden):
    from mgea.decoder import RowSampling
    g, prompts, _ = case(golden, "tiny8h")
    prompts = prompts + [[9, 8, 7]]
    negs = [p[:1] for p in prompts]
    rows = [RowSampling(1.0, 20, seed=7 + b) for b in range(3)]
    eng, _, _ = make(g, max_batch=8)
    fresh, _, _ = make(g, max_batch=8)
    five = prompts + negs[:2]
    rows5 = rows + rows[:2]
    before = eng.generate_rows(five, rows5, N_STEPS).cpu()
    unguided = eng.stats()["graph_instantiates"]
    a = eng.generate_guided(prompts, [negs[0], negs[1], None], rows, [1.5, 3.0, 0.0], N_STEPS, all_rows=True).cpu()   # B = 5
    st = eng.stats()
    inst = st["graph_instantiates"]
    assert inst > unguided, "the guided steps are graphs of their own"
    assert eng.guidance_info() == dict(pairs=2, guided_steps=N_STEPS) and st["graph_replays"] == N_STEPS
    # one launch more than the unguided step of that batch size and form
    eng.generate_rows(five, rows5, 1)
    plain_nodes = eng.stats()["graph_nodes"]
    eng.generate_guided(prompts, [negs[0], negs[1], None], rows, [1.5, 3.0, 0.0], 1)
    assert eng.stats()["graph_nodes"] == plain_nodes + 1
    inst = eng.stats()["graph_instantiates"]
    b = eng.generate_guided(prompts, [None, negs[1], negs[2]], rows, [9.0, 0.5, 2.0], N_STEPS, all_rows=True).cpu()   # B = 5, other pairs
    assert eng.stats()["graph_instantiates"] == inst, "other pairs / scales captured a new guided graph"
    assert torch.equal(b[3], b[1]) and torch.equal(b[4], b[2]) and torch.equal(a[3], a[0]) and torch.equal(a[4], a[1])
    assert not torch.equal(a[:3], b[:3])
    after = eng.generate_rows(five, rows5, N_STEPS).cpu()
    assert eng.stats()["graph_instantiates"] == inst and eng.guidance_info() == dict(pairs=0, guided_steps=0)
    want = fresh.generate_rows(five, rows5, N_STEPS).cpu()
    assert torch.equal(before, want) and torch.equal(after, want), "an unguided call next to a guided one drew other ids"
    # every shadow_row -1 IS the unguided call
    assert torch.equal(eng.generate_guided(five, [None] * 5, rows5, 1.5, N_STEPS).cpu(), want)
    assert eng.stats()["graph_instantiates"] == inst
    eng.close()
    fresh.close()


# ------------------------------------------------------------------------------------- 5. refusals, mixed batches, the window
def raw_guided(eng, prompts, rows, guide, n_steps):
    """mgea_decoder_generate_rows_guided itself on equal-length prompts; returns (status, message, ids)"""
    from mgea import _lib
    from mgea.decoder import pack_rows
    ids = torch.tensor(prompts, dtype=torch.int32, device="cuda")
    B, Tp = ids.shape
    out = torch.empty(B, max(n_steps, 1), dtype=torch.int32, device="cuda")
    recs = pack_rows(rows, eng.vocab, n_steps)
    garr = (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in guide])
    with eng._on_stream():
        rc = eng.lib.mgea_decoder_generate_rows_guided(eng.h, _lib.ptr(ids), None, B, Tp, n_steps, recs, None, None, garr, None, _lib.ptr(out),
                                                       None, None, eng._sp())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), out[:, :n_steps].cpu()


def test_refusals_and_a_mixed_batch(golden):
    from mgea import _lib
    from mgea.decoder import RowSampling
    g, prompts, _ = case(golden, "tiny8h")
    eng, _, _ = make(g, max_batch=5)
    equal = [[5, 6, 7], [8, 9, 10], [11, 12, 13]]
    rows = [RowSampling(1.0, 20, seed=3) for _ in equal]
    for guide, who in (([(3, 1.0), (-1, 0), (-1, 0)], "row 0"), ([(-1, 0), (1, 1.0), (-1, 0)], "row 1"), ([(1, 1.0), (2, 1.0), (-1, 0)], "row 0"),
                       ([(2, 1.0), (2, 1.0), (-1, 0)], "row 1"), ([(-1, 0), (-1, 0), (0, -0.5)], "row 2"), ([(-1, 0), (2, math.inf), (-1, 0)], "row 1"),
                       ([(-2, 1.0), (-1, 0), (-1, 0)], "row 0")):
        rc, msg, _ = raw_guided(eng, equal, rows, guide, 4)
        assert rc == _lib.EINVAL and who in msg, (guide, rc, msg)
    rc, msg, _ = raw_guided(eng, equal, rows, [(2, 1.0), (-1, 0), (-1, 0)], eng.max_ctx)   # capped: 3 + max_ctx > max_ctx
    assert rc == _lib.ECAPACITY and "capped" in msg
    rc, msg, ids = raw_guided(eng, equal, rows, [(-1, 0.0)] * 3, 4)   # every shadow_row -1 IS the unguided call
    assert rc == 0, msg
    assert eng.guidance_info() == dict(pairs=0, guided_steps=0) and torch.equal(ids, eng.generate_rows(equal, rows, 4).cpu())
    with pytest.raises(ValueError, match="never capped"):
        eng.generate_guided(prompts, [p[:1] for p in prompts], rows[:2], 1.5, eng.max_ctx)
    with pytest.raises(ValueError, match="row 2: its shadow row 5 does not fit"):
        eng.generate_guided(equal, [[1], [2], [3]], rows, 1.5, 4)
    with pytest.raises(ValueError, match="row 0: guidance scale"):
        eng.generate_guided(equal, [[1], None, None], rows, -1.0, 4)
    # pairs and an unpaired row: the unpaired one keeps the ids of an unguided sampled-form batch of the same size
    negs = [[5], None, [11]]
    got = eng.generate_guided(equal, negs, rows, 2.0, N_STEPS, all_rows=True).cpu()
    assert got.shape == (5, N_STEPS) and torch.equal(got[3], got[0]) and torch.equal(got[4], got[2])
    plain = eng.generate_rows(equal + [[5], [11]], rows + [rows[0], rows[2]], N_STEPS).cpu()
    assert torch.equal(got[1], plain[1]), "the unpaired row of a guided batch drew other ids than in the unguided batch"
    assert not torch.equal(got[0], plain[0])
    eng.close()


def test_windowed_guided_run_longer_than_the_context():
    from mgea.decoder import RowSampling
    from test_gpu_kv_window import draw_prompts, make as make_windowed, model, want_evictions
    n_steps, max_ctx = 400, 192
    eng = make_windowed("tiny8h", max_ctx, max_batch=4, max_steps=n_steps)
    prompts = draw_prompts(5, model("tiny8h")[2], (5, 9))
    negs = [p[:1] for p in prompts]
    rows = [RowSampling(1.0, 20, seed=11) for _ in prompts]
    ids = eng.generate_guided(prompts, negs, rows, [1.5, 3.0], n_steps, all_rows=True).cpu()
    assert ids.shape == (4, n_steps) and int(ids.min()) >= 0, "a windowed guided run returns n_steps ids"
    assert torch.equal(ids[2], ids[0]) and torch.equal(ids[3], ids[1])
    assert eng.window_evictions() == want_evictions(eng.window, prompts + negs, n_steps)   # every row on the schedule of its own prompt
    assert eng.guidance_info() == dict(pairs=2, guided_steps=n_steps)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the app
def test_guided_endpoint(golden, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_guided_app
    from emotion_analysis import EATS, inference
    from generate_music.guidance import unconditional_prompt
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer

    g = golden("decoder_tiny8h")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))
    monkeypatch.setattr(gen, "_draw_seed", lambda: 1234)   # fixed seeds: the endpoint draws one per request

    with pytest.raises(ValueError, match="guidance_scale"):
        create_guided_app(model, seq_len=32, guidance_scale=-1.0)
    app = create_guided_app(model, seq_len=32, temperature=1.0, top_k=20, guidance_scale=2.0)
    served = []
    app.state.on_tokens = served.append
    client = TestClient(app)
    text = "i am walking down a road and i see a rainbow. i love life."
    kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
    random.seed(11)
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and r.content[:4] == b"MThd" and r.headers["x-guidance-scale"] == "2"
    info = model._need().guidance_info()   # (the steps: all of them, or fewer in whole polls of 16 once the pair has drawn [END_SEQUENCE])
    assert info["pairs"] == 1 and 0 < info["guided_steps"] <= 32 - int(r.headers["x-prompt-tokens"])
    random.seed(11)
    mapping = EATS.get_music_params(r.headers["x-emotion"])
    instruments = [i for fam in mapping["all_families"] for i in gen.FAMILY_TO_INSTRUMENTS.get(fam, [])]
    prompt = ["[START_SEQUENCE]", gen.closest_bpm_token(mapping["bpm"]), gen.normalize_key_signature(mapping["key"])] + \
             [f"[INSTRUMENT] {i}" for i in instruments]
    assert len(unconditional_prompt(prompt)) == len(prompt) - 2
    tokens = gen.sample_kvcache_guided(model, prompt, max_len=32, top_k=20, guidance_scale=2.0)
    assert served == [tokens] and len(tokens) == int(r.headers["x-generated-tokens"]) and tokens[:len(prompt)] == prompt
    # the same seed at another scale, and without guidance, draws another piece; the request's negative prompt is the default one
    assert gen.sample_kvcache_guided(model, prompt, max_len=32, top_k=20, guidance_scale=2.0, negative_prompt=unconditional_prompt(prompt)) == tokens
    assert gen.sample_kvcache_guided(model, prompt, max_len=32, top_k=20, guidance_scale=0.0) != tokens
    two = gen.generate_requests_guided(model, [prompt, prompt], max_len=32, top_k=20, seed=[1234, 5], guidance_scale=[2.0, 1.0])
    assert len(two) == 2 and all(t[:len(prompt)] == prompt for t in two)
