"""The KV window on the MI355X (include/mgea.h, mgea_decoder_set_window): the evict kernel alone against the host rotation, windowed
generations against the oracle driven with the host model's evicted positions masked (teacher-forced log-probabilities, strict
greedy ids), the engine against itself (no window, graphs, batch, EOS, window cleared), the step forms under a window, the fp16
engine, and the drop-in surface.

Geometries: the tiny golden ones (2 layers; tiny8h 256 wide, 8 heads, the fused path; tiny 128 wide, the slab path).  max_ctx 192
is P = 3 pages (plain attention: at most 4 pages), 384 is P = 6 (3 rows x 8 heads: the split attention; 9 rows: plain).

Tolerances: ORACLE_TOL = 2 x parity_util.LOGIT_TOL on a log-probability (one for the logit, one for the log-sum), as
tests/test_gpu_logprobs.py; 2 x test_gpu_f16.F16_LOGIT_TOL for the fp16 engine."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from mgea import synth
from parity_util import LOGIT_TOL, NEAR_TIE

pytestmark = pytest.mark.gpu
ORACLE_TOL = 2 * LOGIT_TOL
EOS = 2
# (max_ctx, prompt lengths, steps, seed of the greedy run): the shapes of the issue
P3 = (192, (5, 9, 2), 400, 4)
P6 = (384, (5, 37, 47), 560, 9)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def model(tag):
    seed, vocab, seq_len, d_model, n_head, n_layer = geometry(tag)
    return synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer), n_head, vocab


def geometry(tag):
    return tuple(int(x) for x in np.load(os.path.join(GOLDEN, f"decoder_{tag}.npz"))["cfg"])


def make(tag, max_ctx, max_batch=4, window=True, max_steps=600, **kw):
    from mgea.decoder import DecoderEngine
    sd, n_head, _ = model(tag)
    eng = DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx, **kw)
    if window:
        eng.set_window(1, None, max_steps=max_steps)
        assert eng.window_info() == eng.window and eng.window.pages == max_ctx // 64
    return eng


def draw_prompts(seed, vocab, lens):
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(0, vocab, n)] for n in lens]


def oracle_windowed(ref, win, prompts, n_steps, forced=None):
    """The reference's loop (prefill, re-feed the last prompt token, one token per step) with cache_valid cleared for the positions
    the host model says are evicted.  forced [B][n_steps] or None (greedy).  Returns ids [B, n], the log-probability (float64
    log_softmax) of every id, and the smallest top-2 logit gap of every step [B, n]."""
    B, lens, Tp = len(prompts), [len(p) for p in prompts], max(len(p) for p in prompts)
    idx = torch.zeros(B, Tp, dtype=torch.long)
    valid = torch.zeros(B, Tp, dtype=torch.bool)
    for b, p in enumerate(prompts):
        idx[b, :len(p)] = torch.tensor(p)
        valid[b, :len(p)] = True
    _, cache, cvalid = ref.forward(idx, None, None, valid)
    last = torch.tensor([p[-1] for p in prompts]).view(B, 1)
    S64 = win.sink_pages * 64
    ids = torch.zeros(B, n_steps, dtype=torch.long)
    lps = torch.zeros(B, n_steps, dtype=torch.float64)
    gaps = torch.zeros(B, n_steps)
    for i in range(n_steps):
        for b in range(B):
            e = win.evictions(lens[b], i)
            if e:   # absolute positions [64 S, 64 (S + e)) of row b; position p >= len sits in column Tp + (p - len)
                cvalid[b, Tp + S64 - lens[b]:Tp + S64 + 64 * e - lens[b]] = False
            assert int(cvalid[b].sum()) + 1 == win.attended_count(lens[b], i)
        logits, cache, cvalid = ref.forward(last, cache, cvalid, None)
        lg = logits[:, -1, :]
        top2 = lg.topk(2, dim=-1).values
        gaps[:, i] = top2[:, 0] - top2[:, 1]
        nxt = lg.argmax(-1) if forced is None else torch.tensor([forced[b][i] for b in range(B)])
        ids[:, i] = nxt
        lps[:, i] = torch.log_softmax(lg.double(), dim=-1)[torch.arange(B), nxt]
        last = nxt.view(B, 1)
    return ids, lps, gaps


@functools.lru_cache(maxsize=None)
def forced_reference(tag, max_ctx, lens, n_steps, rounded=False):
    """The teacher-forced oracle run of a shape, computed once: (prompts, forced ids, oracle log-probabilities, window)."""
    from mgea.decoder import KVWindow
    from oracle.decoder_ref import DecoderRef
    sd, n_head, vocab = model(tag)
    if rounded:
        from test_gpu_f16 import rounded as round_sd
        sd = round_sd(sd)
    win = KVWindow(1, max_ctx // 64 - 1, n_steps)
    prompts = draw_prompts(100 + max_ctx, vocab, lens)
    forced = np.random.default_rng(7 + max_ctx).integers(0, vocab, (len(lens), n_steps)).tolist()
    _, lps, _ = oracle_windowed(DecoderRef(sd, n_head), win, prompts, n_steps, forced)
    return prompts, forced, lps, win


def want_evictions(win, prompts, n_steps):
    return [win.evictions(len(p), n_steps - 1) for p in prompts]


# ------------------------------------------------------------------------------------------------------ 1. the evict op alone
@pytest.mark.parametrize("max_pages", [3, 6, 65, 131, 257])
@pytest.mark.parametrize("S", [1, 2])
def test_evict_op_against_the_host_rotation(max_pages, S):
    from mgea import ops
    from mgea.decoder import KVWindow
    for P in sorted({max_pages, max(S + 2, max_pages - 1)}):   # the whole row, and a window that leaves the last entry outside
        R = P - S
        if R < 2 or P > max_pages:
            with pytest.raises(RuntimeError, match="ring_pages|exceed"):
                ops.window_evict(torch.zeros(1, max_pages, dtype=torch.int32), S, R, torch.zeros(1), torch.zeros(1), torch.zeros(1))
            continue
        trig = 64 * P - 1
        ctx = torch.tensor([trig, trig - 1, trig + 1, trig, trig, 0, trig - 64], dtype=torch.int32)
        done = torch.tensor([0, 0, 0, 1, 0, 0, 2], dtype=torch.int32)
        ev = torch.tensor([0, 5, 6, 7, 41, 0, 3], dtype=torch.int32)
        B = ctx.numel()
        pt = (torch.randperm(B * max_pages, generator=torch.Generator().manual_seed(max_pages * 8 + S)).to(torch.int32) + 1000).view(B, max_pages)
        got = ops.window_evict(pt, S, R, ctx, done, ev)
        want = KVWindow.evict_rows(pt.numpy(), S, R, ctx.numpy(), done.numpy(), ev.numpy())
        for g, w, name in zip(got, want, ("page table", "ctx_len", "evictions")):
            assert torch.equal(g.cpu(), torch.from_numpy(w)), f"max_pages {max_pages} S {S} P {P}: {name}"
        moved = [0, 4]
        assert got[1].cpu().tolist() == [trig - 64 if b in moved else int(ctx[b]) for b in range(B)]
        for b in range(B):
            row, old = got[0][b].cpu(), pt[b]
            if b in moved:
                assert torch.equal(row[:S], old[:S]) and torch.equal(row[P:], old[P:]) and int(row[P - 1]) == int(old[S])
                assert torch.equal(row[S:P - 1], old[S + 1:P])
            else:
                assert torch.equal(row, old), f"row {b} must not move"


def test_evict_op_refuses_a_ring_beyond_its_bound():
    from mgea import ops
    from mgea.decoder import WINDOW_MAX_RING
    z = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=f"ring_pages {WINDOW_MAX_RING + 1} outside"):
        ops.window_evict(torch.zeros(1, WINDOW_MAX_RING + 2, dtype=torch.int32), 1, WINDOW_MAX_RING + 1, z, z, z)
    with pytest.raises(RuntimeError, match="sink_pages 0"):
        ops.window_evict(torch.zeros(1, 8, dtype=torch.int32), 0, 4, z, z, z)


# ------------------------------------------------------------------------------------ 2. teacher-forced scores against the oracle
@pytest.mark.parametrize("max_ctx,lens,n_steps", [P3[:3], P6[:3], (384, (5, 37, 47, 11, 3, 29, 8, 21, 2), 560)],
                         ids=["P3-plain", "P6-split", "P6-9rows-plain"])
def test_teacher_forced_scores_against_the_windowed_oracle(max_ctx, lens, n_steps):
    from mgea.decoder import RowSampling
    prompts, forced, want, win = forced_reference("tiny8h", max_ctx, lens, n_steps)
    eng = make("tiny8h", max_ctx, max_batch=len(lens), max_steps=n_steps)
    res = eng.generate_scored(prompts, [RowSampling(top_k=1) for _ in prompts], n_steps, force_ids=forced)
    assert res.ids.cpu().tolist() == forced
    ev = eng.window_evictions()
    assert ev == want_evictions(win, prompts, n_steps) and min(ev) >= 3, ev
    assert eng.context_lengths().cpu().tolist() == [len(p) + n_steps - 64 * e for p, e in zip(prompts, ev)]
    d = (res.logprobs.cpu().double() - want).abs()
    print(f"[kv window] max_ctx {max_ctx} B {len(lens)}: evictions {ev}, worst |logprob - oracle| {float(d.max()):.2e} "
          f"(before the first eviction {float(d[:, :max_ctx - 1 - max(lens)].max()):.2e})")
    assert float(d.max()) <= ORACLE_TOL, f"step {int(d.max(0).values.argmax())}: {float(d.max()):.2e}"
    eng.close()


# ----------------------------------------------------------------------------------------------------------- 3. greedy ids, strict
@pytest.mark.parametrize("max_ctx,lens,n_steps,seed", [P3, P6], ids=["P3", "P6"])
def test_greedy_ids_equal_the_windowed_oracle(max_ctx, lens, n_steps, seed):
    from mgea.decoder import KVWindow
    from oracle.decoder_ref import DecoderRef
    sd, n_head, vocab = model("tiny8h")
    prompts = draw_prompts(seed, vocab, lens)
    win = KVWindow(1, max_ctx // 64 - 1, n_steps)
    want, _, gaps = oracle_windowed(DecoderRef(sd, n_head), win, prompts, n_steps)
    print(f"[kv window] greedy max_ctx {max_ctx}: the oracle's smallest top-2 gap {float(gaps.min()):.2e}")
    assert float(gaps.min()) >= 2 * NEAR_TIE, "precondition: the oracle's own argmax must be defined at every step"
    eng = make("tiny8h", max_ctx, max_steps=n_steps)
    got = eng.generate(prompts, n_steps, top_k=1).cpu()
    assert eng.window_evictions() == want_evictions(win, prompts, n_steps)
    if not torch.equal(got.long(), want):
        b, i = (int(v) for v in (got.long() != want).nonzero()[0])
        pytest.fail(f"row {b} differs first at step {i} (evictions before it: {win.evictions(lens[b], i)}), oracle gap {float(gaps[b, i]):.2e}")
    eng.close()


# ------------------------------------------------------------------------------------------------- 4. engine against engine, bitwise
def sampled_rows(n, **kw):
    from mgea.decoder import RowSampling
    return [RowSampling(1.0, 50, seed=21, **kw) for _ in range(n)]


def test_short_windowed_generation_equals_the_engine_without_a_window():
    sd, _, vocab = model("tiny8h")
    prompts = draw_prompts(3, vocab, P3[1])
    n = 150   # the longest prompt is 9: the first eviction would open step 182
    win, plain = make("tiny8h", 192), make("tiny8h", 192, window=False)
    for rows in (sampled_rows(3), sampled_rows(3, repetition_penalty=1.2)):
        a, b = win.generate_scored(prompts, rows, n), plain.generate_scored(prompts, rows, n)
        assert torch.equal(a.ids, b.ids) and torch.equal(a.logprobs, b.logprobs) and torch.equal(a.choice_logprobs, b.choice_logprobs)
    assert torch.equal(win.generate(prompts, n, top_k=1), plain.generate(prompts, n, top_k=1))
    assert win.window_evictions() == [0, 0, 0]
    # (e) the windowed greedy step is the unwindowed one behind exactly one more launch
    assert win.stats()["graph_nodes"] == plain.stats()["graph_nodes"] + 1
    with pytest.raises(RuntimeError, match="no window"):
        plain.window_evictions()
    win.close()
    plain.close()


def test_windowed_row_alone_and_in_a_batch(tune):
    """One sampled row past two evictions, alone and as row 0 of three.  Both runs take the same kernels: P = 3 keeps the attention
    plain whatever the batch, and the two switches keep the one-row step off the dot-product kernels and the three-row head off
    the balanced kernel (a row's ids depend on the kernel family)."""
    tune("decoder_nogemv", 1)
    tune("head_balanced", 0)
    sd, _, vocab = model("tiny8h")
    prompts = draw_prompts(5, vocab, (9, 5, 2))
    n = 330
    eng = make("tiny8h", 192)
    three = eng.generate_scored(prompts, sampled_rows(3), n)
    ev3 = eng.window_evictions()
    one = eng.generate_scored(prompts[:1], sampled_rows(1), n)
    assert eng.window_evictions() == ev3[:1] and ev3[0] >= 3
    assert torch.equal(one.ids[0], three.ids[0]) and torch.equal(one.logprobs[0], three.logprobs[0])
    eng.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])   # fused tail with the qkv0 table / slab path with advance_kernel
def test_windowed_graphs_equal_eager_launches(tune, tag):
    _, _, vocab = model(tag)
    prompts = draw_prompts(6, vocab, P3[1])
    n = 340   # 8-step graphs, then the single-step graph for the last four
    runs = []
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng = make(tag, 192)
        res = eng.generate_scored(prompts, sampled_rows(3), n)
        greedy = eng.generate(prompts, n, top_k=1)
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        runs.append((mode, res.ids.cpu(), res.logprobs.cpu(), greedy.cpu(), eng.window_evictions()))
        eng.close()
    assert min(runs[0][4]) >= 3
    for mode, ids, lp, greedy, ev in runs[1:]:
        assert torch.equal(ids, runs[0][1]) and torch.equal(lp, runs[0][2]) and torch.equal(greedy, runs[0][3]) and ev == runs[0][4], \
            f"{tag}: {mode} vs graphs8"


def test_eos_before_and_after_the_first_eviction():
    from mgea.decoder import KVWindow, RowSampling
    _, _, vocab = model("tiny8h")
    prompts = draw_prompts(8, vocab, (5, 9, 2, 7))
    n = 330
    eng = make("tiny8h", 192)
    free = eng.generate_scored(prompts, sampled_rows(4), n)
    ev_free = eng.window_evictions()
    drawn = set(free.ids[[0, 2]].cpu().flatten().tolist())
    eos = next(i for i in range(vocab) if i not in drawn)   # an id rows 0 and 2 never draw by themselves
    forced = [[-1] * 100 + [eos], [], [-1] * 260 + [eos], []]   # row 0 stops before its first eviction (step 186), row 2 after its second
    rows = [RowSampling(1.0, 50, seed=21, eos_id=eos if b in (0, 2) else -1) for b in range(4)]
    res = eng.generate_scored(prompts, rows, n, force_ids=forced)
    ids, ev = res.ids.cpu(), eng.window_evictions()
    win = KVWindow(1, 2, 600)
    for b, stop in ((0, 100), (2, 260)):
        assert int(ids[b, stop]) == eos and bool((ids[b, stop + 1:] == -1).all())
        assert ev[b] == win.evictions(len(prompts[b]), stop), "a finished row's counter stops"
        assert torch.equal(ids[b, :stop], free.ids[b, :stop].cpu())
    assert ev[0] == 0 and ev[2] == 2
    for b in (1, 3):
        assert torch.equal(ids[b], free.ids[b].cpu()) and torch.equal(res.logprobs[b], free.logprobs[b]) and ev[b] == ev_free[b]
    lens = eng.context_lengths().cpu().tolist()
    assert lens[0] == 5 + 101 and lens[2] == 2 + 261 - 128
    eng.close()


def test_clearing_the_window_restores_the_engine():
    _, _, vocab = model("tiny8h")
    prompts = draw_prompts(9, vocab, P3[1])
    eng = make("tiny8h", 192, window=False)
    before = eng.generate_scored(prompts, sampled_rows(3), 100)
    greedy_before = eng.generate(prompts, 100, top_k=1)
    with pytest.raises(ValueError, match="exceeds max_ctx 192"):
        eng.generate(prompts, 400, top_k=1)
    inst = eng.stats()["graph_instantiates"]
    eng.set_window(1, None, max_steps=500)
    long = eng.generate(prompts, 400, top_k=1)
    assert int(long.min()) >= 0 and eng.window_evictions() == [4, 4, 4]
    with pytest.raises(RuntimeError, match="windowed generation"):
        eng.step(None, eng.sampler(1.0, 1))
    with pytest.raises(ValueError, match="max_steps 500"):
        eng.generate(prompts, 501, top_k=1)
    with pytest.raises(ValueError, match="sink"):
        eng.generate([list(range(64))], 10, top_k=1)
    for bad, msg in (((1, 1), "ring_pages 1"), ((2, 2), "sink_pages 2 \\+ ring_pages 2"), ((0 + 1, 2, 0), "max_steps 0")):
        with pytest.raises(ValueError, match=msg):
            eng.set_window(*bad)
    windowed_graphs = eng.stats()["graph_instantiates"] - inst
    eng.set_window(0)
    assert eng.window is None and eng.window_info() is None
    with pytest.raises(ValueError, match="exceeds max_ctx 192"):
        eng.generate(prompts, 400, top_k=1)
    after = eng.generate_scored(prompts, sampled_rows(3), 100)
    assert torch.equal(after.ids, before.ids) and torch.equal(after.logprobs, before.logprobs)
    assert torch.equal(eng.generate(prompts, 100, top_k=1), greedy_before)
    assert eng.stats()["graph_instantiates"] == inst + windowed_graphs, "clearing the window dropped an unwindowed graph"
    eng.close()


def test_absolute_positions_and_the_twin_have_no_window():
    from mgea.decoder import DecoderEngine
    sd, n_head, _ = model("tiny8h")
    for kw in (dict(pos_mode="absolute"), dict(block_mode="twin")):
        eng = DecoderEngine(sd, n_head=n_head, max_batch=2, max_ctx=192, **kw)
        with pytest.raises(ValueError, match="position mode"):
            eng.set_window(1)
        assert eng.lib.mgea_decoder_set_window(eng.h, 1, 2, 10, eng._sp()) == -1   # MGEA_EINVAL from the library itself
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 5. forms compose
def test_forms_compose_under_a_window():
    from mgea.decoder import RowSampling, TokenGrammar
    _, _, vocab = model("tiny8h")
    prompts = draw_prompts(10, vocab, P3[1])
    n = 300
    eng = make("tiny8h", 192)
    # repetition penalty: the bitmaps keep whole-history semantics
    out = eng.generate(prompts, n, top_k=50, seed=3, repetition_penalty=1.3).cpu()
    assert min(eng.window_evictions()) >= 2 and eng.stats()["penalized_steps"] == n
    pres = eng.presence().cpu()
    for b, p in enumerate(prompts):
        want = torch.zeros(vocab, dtype=torch.bool)
        want[torch.tensor(p + out[b].tolist())] = True
        assert torch.equal(pres[b], want), f"row {b}: presence is not the set of all ids seen"
    # logit bias + min_new_tokens
    bias = np.zeros(vocab, np.float32)
    banned = np.arange(40, 140)
    bias[banned] = -np.inf
    out = eng.generate_biased(prompts, n, top_k=50, seed=3, eos_id=EOS, logit_bias=bias, min_new_tokens=280).cpu()
    assert min(eng.window_evictions()) >= 2 and eng.stats()["biased_steps"] > 0
    assert not np.isin(out.numpy(), banned).any(), "a banned id was drawn"
    assert bool((out[:, :280] != EOS).all()) and bool((out[:, :280] >= 0).all()), "min_new_tokens under a window"
    # a two-state grammar: even and odd ids alternate
    gr = TokenGrammar(np.arange(vocab) % 2, [[1, -1], [-1, 0]])
    eng.set_grammar(gr)
    rows = [RowSampling(1.0, 50, seed=3, grammar_state=b % 2) for b in range(3)]
    out = eng.generate_rows(prompts, rows, n).cpu()
    assert min(eng.window_evictions()) >= 2 and eng.grammar_info()["grammar_steps"] == n
    for b in range(3):
        assert gr.accepts(out[b].tolist(), b % 2), f"row {b} left the grammar"
    assert eng.grammar_states().cpu().tolist() == [gr.run(out[b].tolist(), b % 2) for b in range(3)]
    assert eng.id_errors(raise_error=False) == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6. fp16 engine
def test_f16_engine_teacher_forced_against_the_oracle_on_rounded_weights():
    from mgea.decoder import RowSampling
    from test_gpu_f16 import F16_LOGIT_TOL
    max_ctx, lens, n_steps = P3[:3]
    prompts, forced, want, win = forced_reference("tiny8h", max_ctx, lens, n_steps, rounded=True)
    eng = make("tiny8h", max_ctx, max_steps=n_steps, dtype="f16")
    res = eng.generate_scored(prompts, [RowSampling(top_k=1) for _ in prompts], n_steps, force_ids=forced)
    assert eng.window_evictions() == want_evictions(win, prompts, n_steps)
    d = float((res.logprobs.cpu().double() - want).abs().max())
    print(f"[kv window] fp16 engine: worst |logprob - oracle on the rounded matrices| {d:.2e}")
    assert d <= 2 * F16_LOGIT_TOL
    eng.close()


# -------------------------------------------------------------------------------------------------------------------- 7. surface
@pytest.fixture
def drop_in():
    import generate_music.generate as gen
    sd, n_head, vocab = model("tiny8h")
    _, _, seq_len, d_model, _, n_layer = geometry("tiny8h")
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    m = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=4, max_ctx=192)
    m.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}))
    yield gen, m
    m.engine.close()


def test_sample_kvcache_beyond_the_context(drop_in):
    gen, m = drop_in
    names = list(gen.tok2id)
    prompt = ["[START_SEQUENCE]", names[5], names[20], names[34]]
    with pytest.raises(RuntimeError, match="exceeds the engine's reserved context 192"):
        gen.sample_kvcache(m, prompt, max_len=3 * 192, top_k=50, seed=1)
    with pytest.raises(RuntimeError, match="reserved context"):
        gen.score_sequence(m, prompt, names[40:240])
    m.set_window(1)
    toks = gen.sample_kvcache(m, prompt, max_len=3 * 192, top_k=50, seed=1)
    assert toks[:4] == prompt and (len(toks) == 3 * 192 or toks[-1] == "[END_SEQUENCE]")
    assert "[END_SEQUENCE]" not in toks[:-1]
    if len(toks) == 3 * 192:
        assert m.engine.window_evictions() == [m.engine.window.evictions(4, 3 * 192 - 4 - 1)]
    lp = gen.score_sequence(m, prompt, names[40:240])
    assert len(lp) == 200 and all(v < 0 for v in lp)
    # generate_requests: one budget beyond max_ctx and one short (the batcher's call: mgea.serve.RequestBatcher._run)
    outs = gen.generate_requests(m, [prompt, prompt[:3]], max_len=[400, 20], top_k=[50, 1], seed=[1, 2])
    eos = "[END_SEQUENCE]"
    assert (len(outs[0]) == 400 or outs[0][-1] == eos) and (len(outs[1]) == 20 or outs[1][-1] == eos)
    m.set_window(0)
    with pytest.raises(RuntimeError, match="reserved context"):
        gen.generate_requests(m, [prompt], max_len=400)


def test_shim_serves_a_piece_longer_than_the_context(drop_in, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    from api_shim import create_batched_app, create_windowed_app
    from emotion_analysis import inference
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer
    gen, m = drop_in
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))
    monkeypatch.setattr(gen, "_draw_seed", lambda: 1234)
    text = "i am walking down a road and i see a rainbow. i love life."
    for build in (create_windowed_app, create_batched_app):
        app = build(m, seq_len=450, temperature=1.0, top_k=50, window=(1, 2))
        assert m.engine.window.max_steps == 450 and m.engine.window.pages == 3
        served = []
        app.state.on_tokens = served.append
        kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
        random.seed(11)
        r = TestClient(app).post("/generate", **kw)
        assert r.status_code == 200 and r.content[:4] == b"MThd"
        assert len(served[0]) == 450 or served[0][-1] == "[END_SEQUENCE]"
        assert len(served[0]) > 192 or served[0][-1] == "[END_SEQUENCE]"
        if app.state.batcher is not None:
            app.state.batcher.close()
