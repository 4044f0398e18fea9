"""Per-token log-probabilities and forced ids on the MI355X: the scored sampler against float64 at the op level, the engine's
log-probabilities against the reference's own step logits, score() against a teacher-forced oracle loop, bitwise self-consistency
across the graph modes, the generation left as it was, forced prefixes, EOS / budget bookkeeping, graph reuse, the fp16 engine and
the best-of endpoint.

Tolerances: 1e-4 on log-probabilities at the op level (the project's rtol 1e-4 on probabilities, carried to log space; plain fp32
arithmetic of the formula is within 2e-6 of float64, tests/test_logprobs_host.py); 2e-3 = 2 x parity_util.LOGIT_TOL against the
oracle (one for the logit, one for the log-sum); 8e-3 = 2 x test_gpu_f16.F16_LOGIT_TOL for the fp16 engine."""
import math
import random

import numpy as np
import pytest
import torch

from mgea import synth
from parity_util import LOGIT_TOL
from test_gpu_logit_bias import SETTINGS, make_bias
from test_gpu_step_forms import EOS, N_STEPS, case
from test_repetition_penalty_host import penalize

pytestmark = pytest.mark.gpu
NINF = -math.inf
OP_TOL = 1e-4
ORACLE_TOL = 2 * LOGIT_TOL


def make(g, max_batch=4, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    max_ctx = kw.pop("max_ctx", seq_len)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx, **kw), sd, n_head


def oracle_score(ref, prompt, cont):
    """The issue's loop for one row: prefill, re-feed the last prompt token, log_softmax at the continuation id, feed that id."""
    _, cache, valid = ref.forward(torch.tensor([prompt]))
    last = torch.tensor([[prompt[-1]]])
    out = []
    for t in cont:
        logits, cache, valid = ref.forward(last, cache, valid)
        out.append(float(torch.log_softmax(logits[0, -1].double(), dim=0)[t]))
        last = torch.tensor([[t]])
    return out


def ragged_case(rng, vocab, B=3):
    prompts = [[int(v) for v in rng.integers(0, vocab, n)] for n in (3, 6, 4)][:B]
    conts = [[int(v) for v in rng.integers(0, vocab, int(rng.integers(10, 21)))] for _ in range(B)]
    return prompts, conts


# ---------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("V", [100, 8324, 14336])
def test_op_scored_sampler(V):
    from mgea import ops
    from mgea.decoder import RowSampling
    rng = np.random.default_rng(2000 + V)
    B = 4
    raw = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    want_lp = torch.log_softmax(torch.from_numpy(raw).double(), dim=1).numpy()   # the reference, once
    mask = rng.random((B, V)) < 0.2
    kinds = {"none": (None, None, None), "finite": (make_bias(rng, "finite", (B, V)), None, None),
             "ban70": (make_bias(rng, "ban70", (B, V)), None, None), "penalty": (None, mask, 1.3),
             "combined": (make_bias(rng, "mixed", (B, V)), mask, 1.3)}
    dev = torch.from_numpy(raw).cuda()
    rows_ix = np.arange(B)
    worst_lp = worst_ch = 0.0
    for kname, (bias, pmask, pen) in kinds.items():
        pres = None if pmask is None else torch.from_numpy(pmask)
        x = raw if pen is None else penalize(raw, pmask, pen)
        x = x if bias is None else (x + bias).astype(np.float32)
        for temp in (1.0, 0.7):
            for k, tp in SETTINGS:
                label = f"V={V} {kname} T={temp} k={k} top_p={tp}"
                rows = [RowSampling(temp, k, tp, pen, seed=9, logit_bias=None if bias is None else bias[b]) for b in range(B)]
                ids, probs = ops.sample_rows(dev, rows, step=3, want_probs=True, presence=pres)
                ids2, lp, ch, probs2 = ops.sample_rows_scored(dev, rows, step=3, want_probs=True, presence=pres)
                assert torch.equal(ids, ids2) and torch.equal(probs, probs2), label + ": scoring changed the draw"
                i = ids.cpu().numpy()
                p = probs.cpu().numpy().astype(np.float64)
                d_lp = float(np.abs(lp.cpu().numpy() - want_lp[rows_ix, i]).max())
                d_ch = float(np.abs(ch.cpu().numpy() - np.log(p[rows_ix, i])).max())
                worst_lp, worst_ch = max(worst_lp, d_lp), max(worst_ch, d_ch)
                assert d_lp <= OP_TOL, f"{label}: raw logprob off float64 by {d_lp:.2e}"
                assert d_ch <= OP_TOL, f"{label}: choice logprob off log(probs_out) by {d_ch:.2e}"
                if k == 1:
                    assert ch.cpu().tolist() == [0.0] * B, label
                # forced ids: row 0 an id that cannot be drawn (banned, or outside the kept set) where there is one, row 1 free,
                # row 2 the processed argmax, row 3 the last id of the vocabulary
                out0 = np.flatnonzero(p[0] == 0)
                f0 = int(out0[0]) if out0.size else int(raw[0].argmin())
                if bias is not None and np.isinf(bias[0]).any():
                    f0 = int(np.flatnonzero(np.isinf(bias[0]))[0])
                forced = np.array([f0, -1, int(x[2].argmax()), V - 1], np.int32)
                ids3, lp3, ch3, probs3 = ops.sample_rows_scored(dev, rows, step=3, want_probs=True, presence=pres, forced=forced.tolist())
                want_ids = np.where(forced >= 0, forced, i)
                assert ids3.cpu().numpy().tolist() == want_ids.tolist() and torch.equal(probs3, probs), label
                assert float(np.abs(lp3.cpu().numpy() - want_lp[rows_ix, want_ids]).max()) <= OP_TOL, label + ": forced raw logprob"
                pf, got_ch = p[rows_ix, want_ids], ch3.cpu().numpy()
                assert (np.isneginf(got_ch) == (pf == 0)).all(), f"{label}: -inf exactly outside the kept set ({got_ch}, {pf})"
                if out0.size or (bias is not None and np.isinf(bias[0]).any()):
                    assert got_ch[0] == NINF and np.isfinite(lp3.cpu().numpy()[0]), label
                kept = pf > 0
                assert float(np.abs(got_ch[kept] - np.log(pf[kept])).max(initial=0.0)) <= OP_TOL, label + ": forced choice logprob"
    print(f"[logprobs] V={V}: worst |logprob - float64| {worst_lp:.2e}, worst |choice - log(probs_out)| {worst_ch:.2e}")


def test_op_forced_id_beyond_vocab_is_clamped():
    from mgea import ops
    from mgea.decoder import RowSampling
    V = 300
    raw = torch.from_numpy((np.random.default_rng(4).standard_normal((2, V)) * 3).astype(np.float32))
    ids, lp, ch = ops.sample_rows_scored(raw.cuda(), [RowSampling(1.0, None)] * 2, forced=[V + 7, 5])
    assert ids.cpu().tolist() == [V - 1, 5]
    want = torch.log_softmax(raw.double(), dim=1)
    assert abs(float(lp[0]) - float(want[0, V - 1])) <= OP_TOL and abs(float(lp[1]) - float(want[1, 5])) <= OP_TOL


# ---------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_greedy_scored_against_the_reference_numbers(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    eng, _, _ = make(g)
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)]
    n = int(g["step_logits0"].shape[0])
    res = eng.generate_scored(prompts, [RowSampling(top_k=1) for _ in prompts], n)
    want_ids = [g[f"greedy{i}"].tolist()[len(p):len(p) + n] for i, p in enumerate(prompts)]
    assert res.ids.cpu().tolist() == want_ids
    assert torch.equal(res.ids, eng.generate(prompts, n, top_k=1))
    assert eng.stats()["scored_steps"] == 0   # the unscored call after it
    worst = 0.0
    for i in range(3):
        want = torch.log_softmax(torch.from_numpy(g[f"step_logits{i}"]).double(), dim=1)
        want = want[torch.arange(n), torch.tensor(want_ids[i])]
        d = float((res.logprobs[i].cpu().double() - want).abs().max())   # every row, every step
        worst = max(worst, d)
        assert d <= ORACLE_TOL, f"{tag}: row {i} logprobs off the reference's by {d:.2e}"
    assert bool((res.choice_logprobs == 0).all()), "a greedy row keeps its argmax: choice log-probability 0"
    print(f"[logprobs] {tag}: greedy logprobs vs log_softmax(reference step logits): {worst:.2e}")
    eng.close()


@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])   # unfused / fused tail
def test_score_against_the_oracle(golden, tag):
    from oracle.decoder_ref import DecoderRef
    g = golden("decoder_" + tag)
    eng, sd, n_head = make(g)
    prompts, conts = ragged_case(np.random.default_rng(31), eng.vocab)
    lp, sums = eng.score(prompts, conts)
    lp = lp.cpu()
    assert lp.shape == (3, max(len(c) for c in conts))
    ref = DecoderRef(sd, n_head)
    worst = 0.0
    for b in range(3):
        want = torch.tensor(oracle_score(ref, prompts[b], conts[b]), dtype=torch.float64)
        d = float((lp[b, :len(want)].double() - want).abs().max())
        worst = max(worst, d)
        assert d <= ORACLE_TOL, f"{tag}: row {b} off the oracle by {d:.2e}"
        assert bool((lp[b, len(want):] == 0).all())
        assert abs(float(sums[b]) - float(want.sum())) <= ORACLE_TOL * len(want)
    print(f"[logprobs] {tag}: score() vs the teacher-forced oracle: {worst:.2e}")
    eng.close()


@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_score_reproduces_the_generation_bitwise_in_every_graph_mode(golden, tune, tag):
    """generate_scored (sampled) then score(prompts, its ids): same kernels, same inputs, same logprobs -- under 8-step graphs,
    1-step graphs and eager launches, all equal; and a forced prefix of the run's own ids leaves its tail alone."""
    from mgea.decoder import RowSampling
    g, prompts, _ = case(golden, tag)
    rows = [RowSampling(1.0, 20, seed=7) for _ in prompts]
    seen = []
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng, _, _ = make(g)
        res = eng.generate_scored(prompts, rows, N_STEPS)
        assert int(res.ids.min()) >= 0 and eng.stats()["scored_steps"] == N_STEPS
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        lp, _ = eng.score(prompts, res.ids.cpu().tolist())
        assert torch.equal(lp, res.logprobs), f"{tag} {mode}: score() of the run's own ids differs from its logprobs"
        assert bool(torch.isfinite(res.choice_logprobs).all()) and bool((res.choice_logprobs <= 0).all())
        pre = eng.generate_scored(prompts, rows, N_STEPS, force_ids=res.ids[:, :4].cpu().tolist())
        assert torch.equal(pre.ids, res.ids) and torch.equal(pre.logprobs, res.logprobs), f"{tag} {mode}: forced prefix"
        assert torch.equal(pre.choice_logprobs, res.choice_logprobs)
        seen.append((mode, res.ids.cpu(), res.logprobs.cpu(), res.choice_logprobs.cpu()))
        eng.close()
    for mode, ids, lp, ch in seen[1:]:
        assert torch.equal(ids, seen[0][1]) and torch.equal(lp, seen[0][2]) and torch.equal(ch, seen[0][3]), f"{tag}: {mode} vs graphs8"


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_scoring_leaves_the_generation_alone(golden, tag):
    from mgea.decoder import RowSampling
    g, prompts, bias = case(golden, tag)
    eng, _, _ = make(g)
    forms = {"sampled": RowSampling(1.0, 20, seed=7), "penalized": RowSampling(1.0, 20, None, 1.2, seed=7),
             "biased": RowSampling(1.0, 20, None, 1.2, EOS, 0, 7, None, bias, 3), "greedy": RowSampling(1.0, 1)}
    for name, row in forms.items():
        rows = [row for _ in prompts]
        want = eng.generate_rows(prompts, rows, N_STEPS)
        res = eng.generate_scored(prompts, rows, N_STEPS)
        assert torch.equal(res.ids, want), f"{tag}: the scored {name} generation drew other ids"
        live = res.ids >= 0
        assert bool(torch.isfinite(res.logprobs).all()) and bool((res.logprobs[live] < 0).all())
        assert bool((res.logprobs[~live] == 0).all()) and bool((res.choice_logprobs[~live] == 0).all())
    assert torch.equal(eng.generate_scored(prompts, [forms["greedy"]] * 2, N_STEPS).ids, eng.generate(prompts, N_STEPS, top_k=1))
    eng.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_forced_eos_and_budget(golden, tag):
    from mgea.decoder import RowSampling
    g, prompts, _ = case(golden, tag)
    eng, _, _ = make(g)
    rows = [RowSampling(1.0, 20, eos_id=EOS, seed=3), RowSampling(1.0, 20, eos_id=-1, seed=3, max_new_tokens=5)]
    res = eng.generate_scored(prompts, rows, N_STEPS, force_ids=[[7, -1, -1, EOS], []])
    ids, lp, ch = res.ids.cpu(), res.logprobs.cpu(), res.choice_logprobs.cpu()
    assert ids[0, 0] == 7 and ids[0, 3] == EOS and bool((ids[0, 4:] == -1).all()), "a forced eos_id finishes the row"
    assert bool(torch.isfinite(lp[0, :4]).all()) and bool((lp[0, :4] < 0).all())
    assert bool((lp[0, 4:] == 0).all()) and bool((ch[0, 4:] == 0).all())
    assert bool((ids[1, :5] >= 0).all()) and bool((ids[1, 5:] == -1).all()), "the budget finishes the row"
    assert bool((lp[1, :5] < 0).all()) and bool((lp[1, 5:] == 0).all()) and bool((ch[1, 5:] == 0).all())
    # min_new_tokens bans the EOS at step 3; forcing it there: the model's own value is finite, the choice value is -inf
    rows = [RowSampling(1.0, 20, eos_id=EOS, seed=3, min_new_tokens=6), RowSampling(1.0, 20, eos_id=-1, seed=3)]
    res = eng.generate_scored(prompts, rows, N_STEPS, force_ids=[[-1, -1, -1, EOS], []])
    assert int(res.ids[0, 3]) == EOS and bool((res.ids[0, 4:] == -1).all())
    assert math.isfinite(float(res.logprobs[0, 3])) and float(res.choice_logprobs[0, 3]) == NINF
    # a forced id handed over in device memory that lies outside the vocabulary: clamped, and the sticky flag says so
    bad = torch.full((2, N_STEPS), -1, dtype=torch.int32, device="cuda")
    bad[1, 2] = eng.vocab + 5
    res = eng.generate_scored(prompts, rows, N_STEPS, force_ids=bad, check_ids=False)
    assert int(res.ids[1, 2]) == eng.vocab - 1 and eng.id_errors(raise_error=False) & 1
    with pytest.raises(ValueError, match="row 1"):
        eng.generate_scored(prompts, rows, N_STEPS, force_ids=[[1], [eng.vocab]])
    eng.close()


def test_scored_graphs_are_reused_and_leave_the_unscored_ones_alone(golden):
    from mgea.decoder import RowSampling
    g, prompts, bias = case(golden, "tiny8h")
    eng, _, _ = make(g)
    fresh, _, _ = make(g)
    rows = [RowSampling(1.0, 20, None, 1.2, EOS, 0, 7, None, bias, 3) for _ in prompts]
    a = eng.generate_scored(prompts, rows, N_STEPS, force_ids=[[5], []])
    st = eng.stats()
    assert st["scored_steps"] > 0 and st["scored_steps"] == st["graph_replays"]
    inst = st["graph_instantiates"]
    rows2 = [RowSampling(0.9, 10, None, 1.1, EOS, 0, 99, None, -bias, 2) for _ in prompts]
    b = eng.generate_scored(prompts, rows2, N_STEPS, force_ids=[[], [9, 9, 4]])
    assert eng.stats()["graph_instantiates"] == inst, "another seed / forced ids / bias captured a new scored graph"
    assert not torch.equal(a.ids, b.ids) and b.ids[1, :3].cpu().tolist() == [9, 9, 4]
    want = fresh.generate_rows(prompts, rows, N_STEPS)
    got = eng.generate_rows(prompts, rows, N_STEPS)
    assert torch.equal(got, want) and eng.stats()["scored_steps"] == 0
    assert eng.stats()["graph_instantiates"] - inst == fresh.stats()["graph_instantiates"], "the unscored call captured something extra"
    eng.close()
    fresh.close()


def test_f16_engine_score_against_the_oracle_on_rounded_weights(golden):
    from oracle.decoder_ref import DecoderRef
    from test_gpu_f16 import F16_LOGIT_TOL, rounded
    g = golden("decoder_S")
    eng, sd, n_head = make(g, max_ctx=256, dtype="f16")
    prompts, conts = ragged_case(np.random.default_rng(32), eng.vocab)
    conts = [c[:12] for c in conts]
    lp, _ = eng.score(prompts, conts)
    ref = DecoderRef(rounded(sd), n_head)
    worst = 0.0
    for b in range(3):
        want = torch.tensor(oracle_score(ref, prompts[b], conts[b]), dtype=torch.float64)
        worst = max(worst, float((lp[b, :len(want)].cpu().double() - want).abs().max()))
    print(f"[logprobs] fp16 engine: score() vs the oracle on the rounded matrices: {worst:.2e}")
    assert worst <= 2 * F16_LOGIT_TOL
    eng.close()


# ---------------------------------------------------------------------------------------------------------- endpoint
def test_best_of_endpoint(golden, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_best_of_app
    from emotion_analysis import EATS, inference
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

    app = create_best_of_app(model, seq_len=32, temperature=1.0, top_k=20, best_of=3)
    served = []
    app.state.on_tokens = served.append
    client = TestClient(app)
    text = "i am walking down a road and i see a rainbow. i love life."
    kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
    random.seed(11)
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and r.content[:4] == b"MThd"
    assert r.headers["x-best-of"] == "3" and math.isfinite(float(r.headers["x-mean-logprob"]))
    random.seed(11)
    mapping = EATS.get_music_params(r.headers["x-emotion"])
    instruments = [i for fam in mapping["all_families"] for i in gen.FAMILY_TO_INSTRUMENTS.get(fam, [])]
    prompt = ["[START_SEQUENCE]", gen.closest_bpm_token(mapping["bpm"]), gen.normalize_key_signature(mapping["key"])] + \
             [f"[INSTRUMENT] {i}" for i in instruments]
    tokens, cands, means, best = gen.generate_best_of(model, prompt, 3, max_len=32, top_k=20, return_all=True)
    assert len(cands) == 3 and len({tuple(c) for c in cands}) > 1, "the candidates draw from different Philox streams"
    # pick_best over the candidates' own ids and log-probabilities (scored again, in a batch of the same size) names the one served
    eng = model._need()
    pid = [gen.tok2id[t] for t in prompt]
    conts = [[gen.tok2id[t] for t in c[len(prompt):]] for c in cands]
    lp, _ = eng.score([pid] * 3, conts)
    width = lp.shape[1]
    ids = [c + [-1] * (width - len(c)) for c in conts]
    assert best == gen.pick_best(ids, lp.cpu().tolist()) and served == [cands[best]] and tokens == cands[best]
    assert gen.mean_logprobs(ids, lp.cpu().tolist()) == means
    assert abs(float(r.headers["x-mean-logprob"]) - means[best]) < 1e-5
    alone = gen.score_sequence(model, prompt, cands[best][len(prompt):])   # one row: other GEMM kernels, the same model
    assert len(alone) == len(conts[best]) and max(abs(a - b) for a, b in zip(alone, lp[best].cpu().tolist())) <= ORACLE_TOL
