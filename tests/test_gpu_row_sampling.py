"""Per-row sampler records on the MI355X: mgea_op_sample_rows against uniform single-row calls, and mgea_decoder_generate_rows --
row independence (B = 8 and 3, f32 and f16), position independence, greedy rows inside a sampled batch, budgets and the early
stop, the uniform call through the row form, and graph reuse."""
import numpy as np
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu


def make(g, max_batch=8, dtype="f32", max_ctx=None):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, dtype=dtype)


def rand_prompts(rng, B, vocab, lo, hi):
    return [list(rng.integers(0, vocab, int(rng.integers(lo, hi + 1)))) for _ in range(B)]


def mixed_rows(n, **extra):
    """n records cycling through greedy, top-k, top-p, penalized, temperature and greedy + penalty settings"""
    from mgea.decoder import RowSampling
    kinds = [dict(top_k=1), dict(top_k=50, seed=11), dict(top_k=0, top_p=0.92, seed=12), dict(top_k=50, repetition_penalty=1.1, seed=13),
             dict(temperature=0.7, top_k=20, seed=14), dict(top_k=1, repetition_penalty=1.2), dict(top_k=0, top_p=0.9, temperature=1.3,
             repetition_penalty=1.1, seed=15), dict(top_k=0, seed=16)]
    return [RowSampling(**{**kinds[i % len(kinds)], **extra}) for i in range(n)]


def uniform(eng, prompts, r, n):
    """generate() with record r on every row (stream = b, no budget)"""
    return eng.generate(prompts, n, r.temperature, r.top_k, r.top_p, r.eos_id, r.seed, repetition_penalty=r.repetition_penalty).cpu()


# ---------------------------------------------------------------------------------------------------------- op level
def test_op_sample_rows_matches_uniform_single_row_calls():
    from mgea import ops
    from mgea.decoder import RowSampling
    rng = np.random.default_rng(3)
    B, V = 16, 8324
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    x[0, [100, 7000]] = x[0].max() + 1.0          # exact ties at the maximum: the lowest id wins
    x[5, [64, 4000]] = x[5].max() + 1.0
    logits = torch.from_numpy(x).cuda()
    mask = rng.random((B, V)) < 0.2
    mask[5, [64, 4000]] = False                   # (row 5 is penalized: keep its tie)
    kinds = [dict(top_k=1), dict(top_k=50), dict(top_k=0, top_p=0.92), dict(top_k=50, repetition_penalty=1.1),
             dict(temperature=0.7, top_k=0), dict(top_k=1, temperature=0.7, repetition_penalty=1.1), dict(top_k=0, top_p=0.92,
             repetition_penalty=1.1), dict(temperature=0.7, top_k=20, top_p=0.8)]
    rows = [RowSampling(**kinds[b % len(kinds)], seed=1000 + 7 * b, stream=int(rng.integers(0, 6))) for b in range(B)]
    step = 5
    ids, probs = ops.sample_rows(logits, rows, step=step, want_probs=True, presence=torch.from_numpy(mask))
    ids, probs = ids.cpu(), probs.cpu()
    for b, r in enumerate(rows):
        # the same row alone through the uniform op, placed at index `stream` so that its Philox counter is the row's
        S = r.stream + 1
        one = logits[b:b + 1].expand(S, V).contiguous()
        kw = dict(repetition_penalty=r.repetition_penalty, presence=torch.from_numpy(np.repeat(mask[b:b + 1], S, 0))) \
            if r.repetition_penalty else {}
        temp = 1.0 if (r.top_k == 1 and not r.repetition_penalty) else r.temperature   # greedy: no division on the row path
        wid, wp = ops.sample(one, temp, r.top_k, r.top_p, seed=r.seed, step=step, want_probs=True, **kw)
        assert int(ids[b]) == int(wid[r.stream]), f"row {b} ({r})"
        assert np.array_equal(probs[b].numpy().view(np.uint32), wp[r.stream].cpu().numpy().view(np.uint32)), f"row {b} ({r})"
        if r.top_k == 1:   # the exact argmax of the (penalized) row, ties to the lowest id
            y = x[b].copy()
            if r.repetition_penalty:
                p = np.float32(r.repetition_penalty)
                y = np.where(mask[b], np.where(y < 0, y * p, y / p), y).astype(np.float32)
            assert int(ids[b]) == int(np.flatnonzero(y == y.max())[0]), f"row {b}"
    assert int(ids[0]) == 100 and int(ids[5]) == 64


def test_op_sample_rows_bad_records():
    from mgea import ops
    from mgea.decoder import RowSampling
    logits = torch.zeros(2, 100, device="cuda")
    with pytest.raises(ValueError, match="row 1"):
        ops.sample_rows(logits, [RowSampling(), RowSampling(top_k=101)])
    with pytest.raises(ValueError):
        ops.sample_rows(logits, [RowSampling()])


# ---------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("B, dtype", [(8, "f32"), (3, "f32"), (8, "f16")])
def test_rows_are_independent(golden, B, dtype):
    g = golden("decoder_S")
    eng = make(g, max_batch=8, dtype=dtype)
    rng = np.random.default_rng(50 + B)
    prompts = rand_prompts(rng, B, eng.vocab, 4, 12)
    rows = mixed_rows(8)
    rows = rows[:B] if B > 3 else [rows[1], rows[3], rows[0]]   # B = 3: sampled, penalized and greedy rows
    n = 150
    got = eng.generate_rows(prompts, rows, n).cpu()
    assert eng.stats()["penalized_steps"] == n
    for b, r in enumerate(rows):
        want = uniform(eng, prompts, r, n)
        assert torch.equal(got[b], want[b]), f"row {b} ({r}) differs from row {b} of its uniform batch"
    assert torch.equal(eng.generate_rows(prompts, rows, n).cpu(), got)   # same records, same B: bit-identical


def test_position_independence(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    rng = np.random.default_rng(61)
    prompts = rand_prompts(rng, 8, eng.vocab, 4, 12)
    rows = mixed_rows(8)
    req_p, req_r = prompts[2], RowSampling(top_k=50, temperature=0.9, seed=4242, stream=0)
    prompts[0], prompts[5] = req_p, req_p
    rows[0], rows[5] = req_r, req_r
    out = eng.generate_rows(prompts, rows, 120).cpu()
    assert torch.equal(out[0], out[5]), "the same request draws different ids at rows 0 and 5"
    rows[1] = RowSampling(top_k=0, top_p=0.5, seed=9)   # the other rows' records do not matter either
    assert torch.equal(eng.generate_rows(prompts, rows, 120).cpu()[5], out[5])


def test_greedy_rows_inside_a_sampled_batch(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    prompts = [g[f"prompt{i}"].tolist() for i in range(4)]
    n = len(g["greedy0"]) - len(prompts[0])
    greedy = eng.generate(prompts, n, 1.0, 1).cpu()
    rows = [RowSampling(top_k=1, temperature=0.7), RowSampling(top_k=50, seed=3), RowSampling(top_k=1),
            RowSampling(top_k=0, top_p=0.9, seed=4)]
    out = eng.generate_rows(prompts, rows, n).cpu()
    for b in (0, 2):
        assert torch.equal(out[b], greedy[b])
        assert prompts[b] + out[b].tolist() == g[f"greedy{b}"].tolist()
    rows_pen = [RowSampling(top_k=1), RowSampling(top_k=50, seed=3, repetition_penalty=1.1), RowSampling(top_k=1, temperature=1.5),
                RowSampling(top_k=50, seed=4)]
    out = eng.generate_rows(prompts, rows_pen, n).cpu()   # the penalized form: p = 1 rows are unchanged
    for b in (0, 2):
        assert prompts[b] + out[b].tolist() == g[f"greedy{b}"].tolist()


def test_budgets_and_early_stop(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    rng = np.random.default_rng(71)
    prompts = rand_prompts(rng, 4, eng.vocab, 4, 12)
    rows = [RowSampling(top_k=50, seed=1), RowSampling(top_k=1), RowSampling(top_k=0, top_p=0.9, seed=2, repetition_penalty=1.1),
            RowSampling(top_k=20, seed=3)]
    n = 100
    full = eng.generate_rows(prompts, rows, n).cpu()
    assert eng.stats()["graph_replays"] == n
    rows[1].max_new_tokens = 37
    rows[2].max_new_tokens = 37
    got = eng.generate_rows(prompts, rows, n).cpu()
    for b in (1, 2):
        assert torch.equal(got[b, :37], full[b, :37]) and bool((got[b, 37:] == -1).all())
    assert torch.equal(got[0], full[0]) and torch.equal(got[3], full[3])
    lens = eng.context_lengths().cpu().tolist()
    assert lens[1] == len(prompts[1]) + 37 and lens[2] == len(prompts[2]) + 37 and lens[0] == len(prompts[0]) + n
    eos = int(full[0, 10])   # a budget and an EOS id on every row: the call stops early
    for r, k in zip(rows, (30, 37, 20, 25)):
        r.max_new_tokens = k
    rows[0].eos_id = eos
    got = eng.generate_rows(prompts, rows, n).cpu()
    assert eng.stats()["graph_replays"] < n
    assert got[0].tolist().index(eos) <= 10 and bool((got[0, got[0].tolist().index(eos) + 1:] == -1).all())
    for b, k in ((1, 37), (2, 20), (3, 25)):
        assert bool((got[b, :k] >= 0).all()) and bool((got[b, k:] == -1).all())


def test_budgets_past_the_padded_reservation(golden):
    """Ragged prompts whose longest one + n_steps exceeds max_ctx: every row fits its own budget, the reservation is max_ctx."""
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8, max_ctx=128)
    rng = np.random.default_rng(73)
    prompts = [list(rng.integers(0, eng.vocab, k)) for k in (4, 6, 5)]
    rows = [RowSampling(top_k=1, max_new_tokens=128 - len(p)) for p in prompts]
    out = eng.generate_rows(prompts, rows, 124).cpu()
    want = eng.generate([prompts[0]] * 3, 124, 1.0, 1).cpu()
    assert torch.equal(out[0], want[0])
    assert eng.context_lengths().cpu().tolist() == [128, 128, 128]
    for b, p in enumerate(prompts):
        assert bool((out[b, :128 - len(p)] >= 0).all()) and bool((out[b, 128 - len(p):] == -1).all())


@pytest.mark.parametrize("B", [3, 64])
def test_uniform_call_through_the_row_form(golden, B):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=64)
    rng = np.random.default_rng(80 + B)
    prompts = rand_prompts(rng, B, eng.vocab, 4, 12)
    n = 40
    for kw in (dict(top_k=1), dict(top_k=50, seed=5), dict(top_k=0, top_p=0.92, seed=6), dict(top_k=0, top_p=0.92, seed=7,
               repetition_penalty=1.1), dict(top_k=1, repetition_penalty=1.2)):
        r = RowSampling(**kw)
        want = uniform(eng, prompts, r, n)
        assert torch.equal(eng.generate_rows(prompts, [r] * B, n).cpu(), want), kw


def test_mixed_calls_reuse_the_uniform_graphs(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    rng = np.random.default_rng(91)
    prompts = rand_prompts(rng, 4, eng.vocab, 4, 12)
    n = 40
    for uni, mixed, other in (
            (dict(top_k=50, seed=1), [dict(top_k=1), dict(top_k=50, seed=2), dict(top_k=0, top_p=0.9), dict(temperature=0.5)],
             [dict(top_k=20, seed=9), dict(top_k=1, temperature=3.0), dict(top_k=50), dict(top_k=0)]),
            (dict(top_k=50, seed=1, repetition_penalty=1.1), [dict(top_k=1), dict(top_k=50, repetition_penalty=1.3), dict(top_k=0),
             dict(top_k=1, repetition_penalty=1.2)], [dict(top_k=50, repetition_penalty=0.9)] * 4),
            (dict(top_k=1), [dict(top_k=1, seed=3)] * 4, [dict(top_k=1, temperature=0.3, eos_id=5, max_new_tokens=30)] * 4)):
        uniform(eng, prompts, RowSampling(**uni), n)
        inst = eng.stats()["graph_instantiates"]
        eng.generate_rows(prompts, [RowSampling(**k) for k in mixed], n)
        assert eng.stats()["graph_instantiates"] == inst, f"mixed call after {uni} captured a graph"
        eng.generate_rows(prompts, [RowSampling(**k) for k in other], n)
        assert eng.stats()["graph_instantiates"] == inst, f"second mixed call after {uni} captured a graph"


def test_presence_after_a_penalized_row_call(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng = make(g, max_batch=8)
    rng = np.random.default_rng(97)
    prompts = rand_prompts(rng, 3, eng.vocab, 4, 12)
    rows = [RowSampling(top_k=1), RowSampling(top_k=50, seed=2, repetition_penalty=1.3), RowSampling(top_k=0, max_new_tokens=20)]
    out = eng.generate_rows(prompts, rows, 50).cpu()
    pres = eng.presence().cpu().numpy()
    for b, q in enumerate(prompts):
        assert set(np.nonzero(pres[b])[0].tolist()) == set(q) | {i for i in out[b].tolist() if i >= 0}
