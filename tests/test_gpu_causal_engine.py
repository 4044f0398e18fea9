"""The causal mode of the decoder engine (pos_mode="causal": true positions, a causal mask in every prefill, every token fed once) against
CausalRef (tests/causal_util.py), the torch-CPU restatement that test_causal_host.py ties to the golden-pinned oracle.

Engines from synth.decoder_state_dict: `tiny` (d_model 128, 2 heads, 2 layers: the unfused path, decoder_tiny's geometry with a longer
position table), `fused` (d_model 256, 4 heads, 2 layers, vocab 500: the fused path up to 512 rows, run_blocks beyond) and `fused` with
fp16 storage.  f32 unless a test says otherwise."""
import numpy as np
import pytest
import torch

import causal_util as U
from mgea import synth

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3     # the north-star bar
F32_TOL = 2e-4       # what the fp32 paths are held to (tests/test_gpu_decoder.py)
GEO = {"tiny": dict(seed=41, vocab=311, seq_len=256, d_model=128, n_layer=2, n_head=2),
       "fused": dict(seed=42, vocab=500, seq_len=256, d_model=256, n_layer=2, n_head=4)}
MAX_CTX = 384


def _sd(kind):
    g = GEO[kind]
    return synth.decoder_state_dict(g["seed"], g["vocab"], g["seq_len"], g["d_model"], g["n_layer"])


_cache = {}


def engine(kind, pos_mode="causal", dtype="f32"):
    """one engine per (geometry, mode, dtype) for the whole module"""
    from mgea.decoder import DecoderEngine
    key = (kind, pos_mode, dtype)
    if key not in _cache:
        _cache[key] = DecoderEngine(_sd(kind), n_head=GEO[kind]["n_head"], max_batch=8, max_ctx=MAX_CTX, pos_mode=pos_mode, dtype=dtype)
    return _cache[key]


def reference(kind):
    if ("ref", kind) not in _cache:
        _cache[("ref", kind)] = U.CausalRef(_sd(kind), n_head=GEO[kind]["n_head"])
    return _cache[("ref", kind)]


def tokens(kind, B, T, tag="ids"):
    return torch.from_numpy(synth.integers(GEO[kind]["seed"], tag, (B, T), 0, GEO[kind]["vocab"])).long()


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for k, v in list(_cache.items()):
        if k[0] not in ("ref", "ref16"):
            v.close()
    _cache.clear()


KINDS = ["tiny", "fused"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["3x70_ragged", "8x80"])
def test_prefill_logits_against_the_causal_reference(kind, shape):
    """[3, 70] with lengths (70, 33, 1) and [8, 80]: 640 rows, beyond the fused path's 512 (run_blocks on both geometries).
    Observed maxima on MI355X: 1.07e-6 / 1.04e-6 (tiny / fused, [3, 70] ragged), 1.19e-6 / 1.07e-6 ([8, 80])."""
    eng, ref = engine(kind), reference(kind)
    if shape == "8x80":
        idx, lens = tokens(kind, 8, 80), None
    else:
        idx, lens = tokens(kind, 3, 70), torch.tensor([70, 33, 1])
    got = eng.reset_and_prefill(idx, lens).cpu()
    valid = None if lens is None else torch.arange(idx.shape[1])[None, :] < lens[:, None]
    want, _, _ = ref.forward(idx, None, None, valid)
    diff = (got - want).abs()
    if valid is not None:
        diff = diff[valid]
    worst = float(diff.max())
    print(f"[causal prefill] {kind} {shape}: max |logits - CausalRef| = {worst:.3e}")
    assert worst < LOGIT_TOL and worst < F32_TOL


@pytest.mark.parametrize("kind,dtype", [("tiny", "f32"), ("fused", "f32"), ("fused", "f16")])
def test_future_tokens_do_not_matter_bitwise(kind, dtype):
    """The same [B, T] call twice with the tokens behind position t replaced: the same launches on the same shapes, so the logits at
    positions <= t are bit-equal -- and on a pos_mode="absolute" engine (true positions, no mask) they are not: the control."""
    B, T = 3, 80
    idx = tokens(kind, B, T)
    V = GEO[kind]["vocab"]
    for mode in ("causal", "absolute"):
        eng = engine(kind, mode, dtype)
        base = eng.reset_and_prefill(idx).cpu()
        for t in (0, 63, 64, T - 2):
            other = idx.clone()
            other[:, t + 1:] = (other[:, t + 1:] + 17) % V
            lg = eng.reset_and_prefill(other).cpu()
            same = torch.equal(lg[:, :t + 1], base[:, :t + 1])
            if mode == "causal":
                assert same, f"{kind} {dtype}: logits at positions <= {t} changed with the tokens behind them"
                assert not torch.equal(lg[:, t + 1:], base[:, t + 1:])
            else:
                assert not same, f"{kind} {dtype}: an unmasked prefill must see the future (t = {t})"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", [1, 64, 65])
def test_prefills_compose(kind, a):
    """forward(ids[:, :a]) then forward(ids[:, a:]) (paged causal attention, T > 1) against the one-shot forward (dense causal
    attention): logits within 2e-4 (observed 4.8e-7), the argmax equal wherever CausalRef decides by more than 4 x the observed
    difference, the KV pages of the two runs -- K and V of every token of every layer, read back through the page table
    (mgea_decoder_kv_pages) -- within 2e-5, and one further step from either cache within 2e-4."""
    eng, ref = engine(kind), reference(kind)
    B, T = 3, 80
    idx = tokens(kind, B, T, "compose")
    nxt = tokens(kind, B, 1, "compose_next")[:, 0].to(torch.int32)
    samp = eng.sampler(1.0, 1)
    n_layer = GEO[kind]["n_layer"]
    whole = eng.reset_and_prefill(idx).cpu()
    kv_whole = [eng.kv_rows(l, [T] * B) for l in range(n_layer)]
    _, step_whole = eng.step(nxt, samp, want_logits=True)
    eng.reset(B)
    parts = torch.cat([eng.forward(idx[:, :a]).cpu(), eng.forward(idx[:, a:]).cpu()], 1)
    assert eng.context_lengths().cpu().tolist() == [T] * B
    kv_parts = [eng.kv_rows(l, [T] * B) for l in range(n_layer)]
    _, step_parts = eng.step(nxt, samp, want_logits=True)
    worst_kv = 0.0
    for l in range(n_layer):
        for b in range(B):
            for x, y in zip(kv_whole[l][b], kv_parts[l][b]):
                assert x.shape == (T, GEO[kind]["n_head"], GEO[kind]["d_model"] // GEO[kind]["n_head"]) and bool(x.abs().sum() > 0)
                worst_kv = max(worst_kv, float((x - y).abs().max()))
    print(f"[causal compose] {kind} a={a}: max |K, V pages of two forwards - of one| = {worst_kv:.3e}")
    assert worst_kv < 2e-5
    d = float((parts - whole).abs().max())
    print(f"[causal compose] {kind} a={a}: max |two forwards - one| = {d:.3e}")
    assert d < F32_TOL
    want, _, _ = ref.forward(idx)
    srt = want.sort(-1).values
    decided = (srt[..., -1] - srt[..., -2]) > 4 * d
    assert torch.equal(parts.argmax(-1)[decided], whole.argmax(-1)[decided])
    assert float((step_parts.cpu() - step_whole.cpu()).abs().max()) < F32_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_steps_equal_prefill(kind):
    """40 teacher-forced steps behind a 30-token prefill against the one-shot causal prefill's logits at the same positions"""
    eng = engine(kind)
    B, P, S = 2, 30, 40
    idx = tokens(kind, B, P + S, "steps")
    whole = eng.reset_and_prefill(idx).cpu()
    eng.reset_and_prefill(idx[:, :P], want_logits=False)
    samp = eng.sampler(1.0, 1)
    worst = 0.0
    for s in range(S):
        _, lg = eng.step(idx[:, P + s].to(torch.int32), samp, want_logits=True)
        worst = max(worst, float((lg.cpu() - whole[:, P + s]).abs().max()))
    print(f"[causal steps] {kind}: max |step - prefill| over {S} steps = {worst:.3e}")
    assert worst < F32_TOL


def _prompts(kind):
    V = GEO[kind]["vocab"]
    ids = synth.integers(GEO[kind]["seed"], "prompts", (4, 65), 1, V).tolist()
    return [ids[0][:1], ids[1][:2], ids[2][:5], ids[3][:65]]


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_generate_against_the_causal_reference(kind):
    """prompts of 1, 2, 5 and 65 tokens in one ragged batch, then each alone (B = 1: the gemv path); 40 steps, ids exact; the context
    after the call is len - 1 + steps: every token was fed once"""
    eng, ref = engine(kind), reference(kind)
    prompts, n = _prompts(kind), 40
    got = eng.generate(prompts, n, temperature=1.0, top_k=1).cpu().tolist()
    assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + n for p in prompts]
    U.diagnose_greedy(eng, ref, prompts, n, got, f"{kind} ragged batch")
    for p in prompts:
        solo = eng.generate([p], n, temperature=1.0, top_k=1).cpu().tolist()
        assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + n]
        U.diagnose_greedy(eng, ref, [p], n, solo, f"{kind} prompt of {len(p)} alone")


def test_greedy_generate_300_steps_past_the_position_table():
    """fused geometry: 300 steps from prompts of 5 and 65 tokens cross several KV pages and run past the table's 256 rows (positions
    clamp to its last row, in the engine and in CausalRef alike)"""
    eng, ref = engine("fused"), reference("fused")
    prompts, n = _prompts("fused")[2:], 300
    got = eng.generate(prompts, n, temperature=1.0, top_k=1).cpu().tolist()
    assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + n for p in prompts]
    U.diagnose_greedy(eng, ref, prompts, n, got, "fused 300 steps")


@pytest.mark.parametrize("kind", KINDS)
def test_sampled_rows_in_a_ragged_batch_equal_their_solo_runs(kind):
    from mgea.decoder import RowSampling
    eng = engine(kind)
    prompts, n = _prompts(kind), 24
    rows = [RowSampling(temperature=0.9, top_k=20, seed=1234, stream=b) for b in range(len(prompts))]
    got = eng.generate_rows(prompts, rows, n).cpu()
    for b, p in enumerate(prompts):
        solo = eng.generate_rows([p], [rows[b]], n).cpu()
        assert torch.equal(solo[0], got[b]), f"{kind}: row {b} (prompt of {len(p)}) differs from its solo run"


@pytest.mark.parametrize("kind", KINDS)
def test_scored_generation_equals_score_prefill(kind):
    """generate_scored's raw log-probabilities (one decode step per token) against score_prefill of what it generated (one masked
    prefill): both sides are held to the 2e-4 logits bar and a log-softmax moves by at most twice a logit perturbation: 4e-4."""
    from mgea.decoder import RowSampling
    eng = engine(kind)
    prompts, n = _prompts(kind), 24
    rows = [RowSampling(temperature=1.0, top_k=30, seed=77, stream=b) for b in range(len(prompts))]
    res = eng.generate_scored(prompts, rows, n)
    conts = res.ids.cpu().tolist()
    lp, tot = eng.score_prefill(prompts, conts)
    d = float((lp.cpu() - res.logprobs.cpu()).abs().max())
    print(f"[causal score] {kind}: max |score_prefill - generate_scored| = {d:.3e}")
    assert d < 4e-4
    assert torch.allclose(tot.cpu(), lp.cpu().sum(1))
    # chunked (a cap of one row's logits) = unchunked, and = the step-by-step score()
    eng.SCORE_PREFILL_LOGITS_BYTES = 1
    try:
        lp1, _ = eng.score_prefill(prompts, conts)
    finally:
        del eng.SCORE_PREFILL_LOGITS_BYTES
    assert float((lp1.cpu() - lp.cpu()).abs().max()) < F32_TOL
    lps, _ = eng.score(prompts, conts)
    assert float((lps.cpu() - lp.cpu()).abs().max()) < 4e-4


def test_score_prefill_past_the_position_table_scores_step_by_step():
    """a row of more than seq_len tokens: one forward cannot take it (the position table), the steps clamp positions: score_prefill
    hands such a call to score() and returns its values"""
    eng = engine("tiny")
    n = GEO["tiny"]["seq_len"]
    prompt = _prompts("tiny")[3][:40]
    cont = tokens("tiny", 1, n, "long_cont")[0].tolist()[:n - 20]          # 40 + 236 = 276 > 256 = seq_len, <= max_ctx
    lp, tot = eng.score_prefill([prompt], [cont])
    want, _ = eng.score([prompt], [cont])
    assert torch.equal(lp.cpu(), want.cpu()) and bool(torch.isfinite(tot).all())
    # and just inside the table the one-pass form agrees with the steps
    lp1, _ = eng.score_prefill([prompt], [cont[:n - 40]])
    w1, _ = eng.score([prompt], [cont[:n - 40]])
    assert float((lp1.cpu() - w1.cpu()).abs().max()) < 4e-4


def reference16():
    """the model the fp16 engine serves: CausalRef on the `fused` weights with the five matrix kinds rounded to fp16 (test_gpu_f16.rounded)"""
    from test_gpu_f16 import rounded
    if ("ref16", "fused") not in _cache:
        _cache[("ref16", "fused")] = U.CausalRef(rounded(_sd("fused")), n_head=GEO["fused"]["n_head"])
    return _cache[("ref16", "fused")]


def test_f16_prefill_logits_against_the_rounded_causal_reference():
    """the fp16 causal engine's numbers: an fp32 dense causal prefill on fp16 matrices, [3, 70] ragged (70, 33, 1), held to
    test_gpu_f16.F16_LOGIT_TOL against the oracle on the rounded weights.  Observed on MI355X: 7.3e-4."""
    from test_gpu_f16 import F16_LOGIT_TOL
    eng, ref = engine("fused", dtype="f16"), reference16()
    idx, lens = tokens("fused", 3, 70), torch.tensor([70, 33, 1])
    got = eng.reset_and_prefill(idx, lens).cpu()
    valid = torch.arange(70)[None, :] < lens[:, None]
    want, _, _ = ref.forward(idx, None, None, valid)
    worst = float((got - want).abs()[valid].max())
    print(f"[causal f16] prefill 3x70 ragged: max |logits - CausalRef(rounded)| = {worst:.3e}")
    assert worst < F16_LOGIT_TOL


@pytest.mark.parametrize("a", [64, 65])
def test_f16_prefills_compose_each_side_against_the_oracle(a):
    """forward(ids[:, :a]) then forward(ids[:, a:]) -- the fp16 causal PAGED kernel extending fp16 pages that the fp32 dense causal
    prefill wrote -- and the one-shot forward, each against the oracle on the rounded weights (the two runs differ from each other by
    the rounding of the first a tokens' K and V, so they are not compared at an fp32 bound), and one further step from either cache.
    Observed on MI355X: 7.3e-4 for one forward and for two (a = 64 and 65), 4.5e-4 .. 5.1e-4 for the step behind them."""
    from test_gpu_f16 import F16_LOGIT_TOL
    eng, ref = engine("fused", dtype="f16"), reference16()
    B, T = 3, 80
    idx = tokens("fused", B, T, "compose")
    nxt = tokens("fused", B, 1, "compose_next")[:, 0]
    want, cache, valid = ref.forward(idx)
    want_step, _, _ = ref.forward(nxt.view(B, 1), cache, valid)
    samp = eng.sampler(1.0, 1)
    whole = eng.reset_and_prefill(idx).cpu()
    _, step_whole = eng.step(nxt.to(torch.int32), samp, want_logits=True)
    eng.reset(B)
    parts = torch.cat([eng.forward(idx[:, :a]).cpu(), eng.forward(idx[:, a:]).cpu()], 1)
    assert eng.context_lengths().cpu().tolist() == [T] * B
    _, step_parts = eng.step(nxt.to(torch.int32), samp, want_logits=True)
    d = {"one forward": float((whole - want).abs().max()), "two forwards": float((parts - want).abs().max()),
         "step behind one": float((step_whole.cpu() - want_step[:, -1]).abs().max()),
         "step behind two": float((step_parts.cpu() - want_step[:, -1]).abs().max())}
    print(f"[causal f16] compose a={a}: max |logits - CausalRef(rounded)|: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert max(d.values()) < F16_LOGIT_TOL, d
    assert not torch.equal(parts[:, a:], whole[:, a:]), "the paged form read the same K and V as the dense one: no fp16 page was read"


def test_f16_teacher_forced_steps_against_the_rounded_causal_reference():
    """40 teacher-forced steps through generate_scored(force_ids = the oracle's greedy ids) behind the ragged prompts of 1, 2, 5 and 65
    tokens: raw log-probabilities within 2 x F16_LOGIT_TOL of the oracle on the rounded weights (one bound for the logit, one for the
    log-sum, as test_gpu_logprobs) -- and, the control of the reference-mode test, more than 1e-4 from the UNROUNDED model's: the mode
    is not a no-op.  Observed on MI355X: 3.7e-4 against the rounded model, 4.6e-4 against the unrounded one."""
    from mgea.decoder import RowSampling
    from test_gpu_f16 import F16_LOGIT_TOL
    eng, ref = engine("fused", dtype="f16"), reference16()
    prompts, n = _prompts("fused"), 40
    outs, sl = ref.generate_greedy(prompts, n, return_logits=True)
    forced = [o[len(p):] for o, p in zip(outs, prompts)]
    res = eng.generate_scored(prompts, [RowSampling(top_k=1, eos_id=-1) for _ in prompts], n, force_ids=forced)
    assert res.ids.cpu().tolist() == forced
    assert eng.context_lengths().cpu().tolist() == [len(p) - 1 + n for p in prompts]
    got = res.logprobs.cpu().double()
    want = torch.log_softmax(sl.double(), -1).gather(2, torch.tensor(forced)[..., None])[..., 0]
    d = float((got - want).abs().max())
    sl32 = U.causal_step_logits(reference("fused"), prompts, forced)
    want32 = torch.log_softmax(sl32.double(), -1).gather(2, torch.tensor(forced)[..., None])[..., 0]
    d32 = float((got - want32).abs().max())
    print(f"[causal f16] 4 rows x {n} teacher-forced steps: max |logprob - oracle(rounded)| = {d:.3e}, against the unrounded model {d32:.3e}")
    assert d <= 2 * F16_LOGIT_TOL
    assert d32 > 1e-4


def test_f16_causal_engine_never_takes_the_16_bit_prefill():
    """[64, 1024] on d_model 256 is the smallest request the fp16 matrix-core prefill takes at its default threshold (256 tiles of
    256 x 256); a causal engine keeps it on the fp32-activation path, whose attention has the causal form: stats[5] stays 0"""
    from mgea.decoder import DecoderEngine
    sd = synth.decoder_state_dict(43, 300, 1024, 256, 2)
    idx = torch.from_numpy(synth.integers(43, "p16", (64, 1024), 0, 300)).to(torch.int32)
    for mode, want in (("reference", 1), ("causal", 0)):
        eng = DecoderEngine(sd, n_head=4, max_batch=64, max_ctx=1024, dtype="f16", pos_mode=mode)
        eng.reset_and_prefill(idx, want_logits=False)
        torch.cuda.synchronize()
        assert eng.stats()["prefill16_forwards"] == want, f"{mode}: prefill16_forwards"
        eng.close()


def test_refusals_launch_nothing():
    from mgea.decoder import DecoderEngine, RowSampling, RowSchedule
    eng = engine("fused")
    before = eng.stats()
    p = [5, 6, 7]
    with pytest.raises(RuntimeError, match="no prompt schedules"):
        eng.generate_scheduled([[p, p]], [RowSampling(top_k=1)], [RowSchedule((2,))], 4)
    with pytest.raises(ValueError, match="window"):
        eng.set_window(1, 2)
    with pytest.raises(RuntimeError, match="MGEA_POS_CAUSAL"):
        DecoderEngine(_sd("fused"), n_head=4, max_batch=2, block_mode="twin", pos_mode="causal")
    with pytest.raises(ValueError, match="pos_mode"):
        DecoderEngine(_sd("fused"), n_head=4, max_batch=2, pos_mode="rope")
    with pytest.raises(ValueError, match="causal"):
        engine("fused", "reference").score_prefill([p], [[1, 2]])
    from generate_music.generate import GPTWithKV
    g = GEO["fused"]
    with pytest.raises(ValueError, match="causal model has no KV window"):     # before an engine exists
        GPTWithKV(g["vocab"], g["seq_len"], g["d_model"], g["n_head"], g["n_layer"], causal=True).set_window(1, 2)
    after = eng.stats()
    assert after["graph_replays"] == before["graph_replays"] and after["graph_instantiates"] == before["graph_instantiates"]


def test_reference_mode_engine_is_what_it_was(golden):
    """in the same process, after causal engines ran: decoder_tiny's golden ids, its contexts with the re-fed token, no 16-bit prefill"""
    from mgea.decoder import DecoderEngine
    engine("tiny").generate([[1, 2, 3]], 4, top_k=1)
    g = golden("decoder_tiny")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    eng = DecoderEngine(synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer), n_head=n_head, max_batch=8, max_ctx=seq_len)
    n = sum(1 for k in g.files if k.startswith("prompt"))
    prompts = [g[f"prompt{i}"].tolist() for i in range(n)]
    steps = len(g["greedy0"]) - len(prompts[0])
    out = eng.generate(prompts, steps, temperature=1.0, top_k=1).cpu()
    for i, p in enumerate(prompts):
        assert p + out[i].tolist() == g[f"greedy{i}"].tolist()
    assert eng.context_lengths().cpu().tolist() == [len(p) + steps for p in prompts]
    lg = eng.reset_and_prefill(torch.tensor([prompts[0]])).cpu()
    assert np.abs(lg[0].numpy() - g["prefill_logits0"]).max() < 5e-5
    assert eng.stats()["prefill16_forwards"] == 0 and not eng.causal
    eng.close()
